// C ABI of libvstab_hip.so (include/vstab.h): context, errors, roctx ranges and the thin wrappers around single launches (glue, warps,
// samplers, clip-driver pieces, post-filters).  The FlowNetS pyramid lives in flownet_plan.cpp / flownet_forward.cpp, the
// VGG16 trunk in vgg_api.cpp, the NLDF head in nldf_api.cpp, the training blocks in train_api.cpp.
#include <cmath>
#include <cstdlib>
#include <new>
#include <vector>

#include "api_internal.h"

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

// ------------------------------------------------------------------------- secondary samplers
extern "C" int vstab_st_transform(const float *img, int B, int H, int W, int C, const float *theta, int theta_dim,
                                  float *out, int oh, int ow, void *stream)
{
    if (!img || !theta || !out) return fail(nullptr, VSTAB_E_STATE, "st_transform: NULL buffer");
    if (B < 1 || H < 1 || W < 1 || C < 1 || oh < 1 || ow < 1 || (theta_dim != 6 && theta_dim != 8))
        return fail(nullptr, VSTAB_E_SHAPE, "st_transform: bad shape (theta must be [B,6] or [B,8])");
    HIP_TRY(nullptr, launch_st_transform(img, B, H, W, C, theta, theta_dim, out, oh, ow, (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" int vstab_st_bilinear_interp(const float *img, int B, int H, int W, int C, const float *x, const float *y,
                                        int oh, int ow, float *out, void *stream)
{
    if (!img || !x || !y || !out) return fail(nullptr, VSTAB_E_STATE, "st_bilinear_interp: NULL buffer");
    if (B < 1 || H < 1 || W < 1 || C < 1 || oh < 1 || ow < 1 || (long long)oh * ow > 0x7fffffffLL)
        return fail(nullptr, VSTAB_E_SHAPE, "st_bilinear_interp: bad shape");
    HIP_TRY(nullptr, launch_st_interp(img, B, H, W, C, x, y, oh, ow, out, (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" int vstab_st_meshgrid(float *out, int oh, int ow, void *stream)
{
    if (!out) return fail(nullptr, VSTAB_E_STATE, "st_meshgrid: NULL buffer");
    if (oh < 1 || ow < 1 || (long long)oh * ow > 0x7fffffffLL / 3) return fail(nullptr, VSTAB_E_SHAPE, "st_meshgrid: bad shape");
    HIP_TRY(nullptr, launch_st_meshgrid(out, oh, ow, (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" int vstab_homography_warp(const float *img, int B, int Hi, int Wi, int C, const float *M, float *out, int oh,
                                     int ow, void *stream)
{
    if (!img || !M || !out) return fail(nullptr, VSTAB_E_STATE, "homography_warp: NULL buffer");
    if (B < 1 || Hi < 1 || Wi < 1 || C < 1 || oh < 1 || ow < 1) return fail(nullptr, VSTAB_E_SHAPE, "homography_warp: bad shape");
    HIP_TRY(nullptr, launch_homography_warp(img, B, Hi, Wi, C, M, out, oh, ow, (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" int vstab_transform_image(const float *img, int B, int Hi, int Wi, int C, const float *ref, const float *pM, float *out, int oh,
                                     int ow, void *stream)
{
    if (!img || !ref || !pM || !out) return fail(nullptr, VSTAB_E_STATE, "transform_image: NULL buffer");
    if (B < 1 || Hi < 1 || Wi < 1 || C < 1 || oh < 1 || ow < 1) return fail(nullptr, VSTAB_E_SHAPE, "transform_image: bad shape");
    HIP_TRY(nullptr, launch_homography_warp(img, B, Hi, Wi, C, pM, out, oh, ow, (hipStream_t)stream, ref));
    return VSTAB_OK;
}

// the rest of spatial_transformer.py's 2-D samplers: bicubic_interp, the symmetric-pad transformers, ElasticTransformer
static bool stx_shape_ok(int B, int H, int W, int C, int oh, int ow)
{
    return B >= 1 && B <= 65535 && H >= 1 && W >= 1 && C >= 1 && oh >= 1 && ow >= 1 && (long long)oh * ow <= 0x7fffffffLL / 4 &&
           (long long)H * W <= 0x7fffffffLL;
}

extern "C" int vstab_st_bicubic_interp(const float *img, int B, int H, int W, int C, const float *x, const float *y, int oh, int ow,
                                       float *out, void *stream)
{
    if (!img || !x || !y || !out) return fail(nullptr, VSTAB_E_STATE, "st_bicubic_interp: NULL buffer");
    if (!stx_shape_ok(B, H, W, C, oh, ow)) return fail(nullptr, VSTAB_E_SHAPE, "st_bicubic_interp: bad shape");
    HIP_TRY(nullptr, launch_st_bicubic_interp(img, B, H, W, C, x, y, oh, ow, out, (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" int vstab_st_transform_interp(const float *img, int B, int H, int W, int C, const float *theta, int theta_dim, int interp,
                                         float *out, int oh, int ow, void *stream)
{
    if (!img || !theta || !out) return fail(nullptr, VSTAB_E_STATE, "st_transform_interp: NULL buffer");
    if (!stx_shape_ok(B, H, W, C, oh, ow) || (theta_dim != 6 && theta_dim != 8))
        return fail(nullptr, VSTAB_E_SHAPE, "st_transform_interp: bad shape (theta must be [B,6] or [B,8])");
    if (interp != VSTAB_INTERP_BILINEAR && interp != VSTAB_INTERP_BICUBIC) return fail(nullptr, VSTAB_E_SHAPE, "st_transform_interp: unknown interp %d", interp);
    HIP_TRY(nullptr, launch_st_transform_interp(img, B, H, W, C, theta, theta_dim, interp, out, oh, ow, (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" int vstab_st_symmetry_transform(const float *img, int B, int H, int W, int C, const float *theta, int kind, int interp,
                                           float *out, int oh, int ow, void *stream)
{
    if (!img || !theta || !out) return fail(nullptr, VSTAB_E_STATE, "st_symmetry_transform: NULL buffer");
    if (oh < 1 || ow < 1 || oh > (1 << 20) || ow > (1 << 20) || !stx_shape_ok(B, H, W, C, oh + 200, ow + 200))
        return fail(nullptr, VSTAB_E_SHAPE, "st_symmetry_transform: bad shape");
    if (H < 100 || W < 100)          // tf.pad SYMMETRIC of 100 px needs H, W >= 100
        return fail(nullptr, VSTAB_E_SHAPE, "st_symmetry_transform: the 100-pixel symmetric pad needs H, W >= 100 (got %dx%d)", H, W);
    if (kind != VSTAB_SYM_AFFINE && kind != VSTAB_SYM_PROJECTIVE && kind != VSTAB_SYM_SIMILARITY)
        return fail(nullptr, VSTAB_E_SHAPE, "st_symmetry_transform: unknown kind %d", kind);
    if (interp != VSTAB_INTERP_BILINEAR && interp != VSTAB_INTERP_BICUBIC) return fail(nullptr, VSTAB_E_SHAPE, "st_symmetry_transform: unknown interp %d", interp);
    HIP_TRY(nullptr, launch_st_symmetry_transform(img, B, H, W, C, theta, kind, interp, out, oh, ow, (hipStream_t)stream));
    return VSTAB_OK;
}

// ElasticTransformer._initialize_tps (ST:187-225) in double: L (K+3)x(K+3) from the fp32 linspace control points, inverted by
// Gauss-Jordan with partial pivoting, transpose(L_inv[:,3:]) rounded to fp32 into linv_t [K, K+3]
extern "C" int vstab_host_tps_linv(int g, float *linv_t, int cap)
{
    if (!linv_t) return fail(nullptr, VSTAB_E_STATE, "host_tps_linv: linv_t is NULL");
    if (g < 2 || g > VSTAB_TPS_GMAX) return fail(nullptr, VSTAB_E_SHAPE, "host_tps_linv: grid side %d outside [2, %d] (g = 1 makes L singular)", g, VSTAB_TPS_GMAX);
    const int K = g * g, N = K + 3;
    if (cap < K * N) return fail(nullptr, VSTAB_E_NOMEM, "host_tps_linv: need %d floats", K * N);
    std::vector<double> px(K), py(K);
    const float step = 2.0f / (float)(g - 1);          // tf.linspace(-1, 1, g) in fp32
    for (int k = 0; k < K; ++k) { px[k] = (double)(-1.0f + (float)(k % g) * step); py[k] = (double)(-1.0f + (float)(k / g) * step); }
    std::vector<double> A((size_t)N * 2 * N, 0.0);     // [L | I]
    auto L = [&](int r, int c) -> double & { return A[(size_t)r * 2 * N + c]; };
    for (int k = 0; k < K; ++k) { L(0, 3 + k) = px[k]; L(1, 3 + k) = py[k]; }
    for (int c = 2; c < N; ++c) L(2, c) = 1.0;         // row 2: [0, 0, 1, ..., 1] (ST:208)
    for (int i = 0; i < K; ++i) {
        L(3 + i, 0) = px[i]; L(3 + i, 1) = py[i]; L(3 + i, 2) = 1.0;
        for (int j = 0; j < K; ++j) {
            const double dx = px[i] - px[j], dy = py[i] - py[j], r2 = dx * dx + dy * dy;
            L(3 + i, 3 + j) = r2 == 0.0 ? 0.0 : r2 * std::log(r2);
        }
    }
    for (int r = 0; r < N; ++r) L(r, N + r) = 1.0;
    for (int c = 0; c < N; ++c) {
        int piv = c;
        for (int r = c + 1; r < N; ++r) if (std::fabs(L(r, c)) > std::fabs(L(piv, c))) piv = r;
        if (std::fabs(L(piv, c)) < 1e-300) return fail(nullptr, VSTAB_E_SHAPE, "host_tps_linv: L is singular");
        if (piv != c) for (int k = 0; k < 2 * N; ++k) std::swap(L(c, k), L(piv, k));
        const double d = L(c, c);
        for (int k = 0; k < 2 * N; ++k) L(c, k) /= d;
        for (int r = 0; r < N; ++r) {
            if (r == c || L(r, c) == 0.0) continue;
            const double f = L(r, c);
            for (int k = 0; k < 2 * N; ++k) L(r, k) -= f * L(c, k);
        }
    }
    for (int k = 0; k < K; ++k)                          // linv_t[k, j] = L_inv[j, 3 + k]
        for (int j = 0; j < N; ++j) linv_t[(size_t)k * N + j] = (float)L(j, N + 3 + k);
    return VSTAB_OK;
}

extern "C" int vstab_st_elastic_transform(const float *img, int B, int H, int W, int C, const float *theta, int g, const float *linv_t,
                                          int interp, float *out, int oh, int ow, void *stream)
{
    if (!img || !theta || !linv_t || !out) return fail(nullptr, VSTAB_E_STATE, "st_elastic_transform: NULL buffer");
    if (!stx_shape_ok(B, H, W, C, oh, ow) || g < 2 || g > VSTAB_TPS_GMAX)
        return fail(nullptr, VSTAB_E_SHAPE, "st_elastic_transform: bad shape (grid side must be in [2, %d])", VSTAB_TPS_GMAX);
    if (interp != VSTAB_INTERP_BILINEAR && interp != VSTAB_INTERP_BICUBIC) return fail(nullptr, VSTAB_E_SHAPE, "st_elastic_transform: unknown interp %d", interp);
    HIP_TRY(nullptr, launch_st_elastic_transform(img, B, H, W, C, theta, g, linv_t, interp, out, oh, ow, (hipStream_t)stream));
    return VSTAB_OK;
}

// ---- backward of the bilinear sampler (sampler_ops.hip): d img by float atomics, d theta by a reproducible two-stage sum
extern "C" size_t vstab_st_transform_backward_workspace_bytes(int B, int H, int W, int C, int oh, int ow)
{
    if (!stx_shape_ok(B, H, W, C, oh, ow)) return 0;
    return st_transform_backward_ws_bytes(B, H, W, C, oh, ow);
}

static bool interp_ok(int interp) { return interp == VSTAB_INTERP_BILINEAR || interp == VSTAB_INTERP_BICUBIC; }

// One set of checks, in one order, for an entry point and its _interp_ form (`name` is the one called): the backward of either sampler
static int st_transform_backward_checked(const char *name, const float *img, int B, int H, int W, int C, const float *theta, int theta_dim,
                                         int interp, const float *dout, int oh, int ow, float *d_img, int accumulate, float *d_theta,
                                         void *workspace, size_t workspace_bytes, void *stream)
{
    if (!img || !theta || !dout) return fail(nullptr, VSTAB_E_STATE, "%s: NULL buffer", name);
    if (!stx_shape_ok(B, H, W, C, oh, ow) || (long long)B * H * W * C > 0x7fffffffLL || (theta_dim != 6 && theta_dim != 8))
        return fail(nullptr, VSTAB_E_SHAPE, "%s: bad shape (theta must be [B,6] or [B,8], B <= 65535)", name);
    if (!interp_ok(interp)) return fail(nullptr, VSTAB_E_SHAPE, "%s: unknown interp %d", name, interp);
    if (!d_img && !d_theta) return fail(nullptr, VSTAB_E_SHAPE, "%s: d_img and d_theta are both NULL", name);
    if (d_theta) {
        const size_t need = st_transform_backward_ws_bytes(B, H, W, C, oh, ow);
        if (!workspace || workspace_bytes < need) return fail(nullptr, VSTAB_E_NOMEM, "%s: workspace needs %zu bytes", name, need);
        if ((uintptr_t)workspace & 7) return fail(nullptr, VSTAB_E_ALIGN, "%s: workspace must be 8-byte aligned", name);
    }
    HIP_TRY(nullptr, launch_st_transform_backward(img, B, H, W, C, theta, theta_dim, dout, oh, ow, d_img, accumulate ? 1 : 0, d_theta,
                                                  (double *)workspace, (hipStream_t)stream, interp));
    return VSTAB_OK;
}

extern "C" int vstab_st_transform_backward(const float *img, int B, int H, int W, int C, const float *theta, int theta_dim, const float *dout,
                                           int oh, int ow, float *d_img, int accumulate, float *d_theta, void *workspace,
                                           size_t workspace_bytes, void *stream)
{
    return st_transform_backward_checked("st_transform_backward", img, B, H, W, C, theta, theta_dim, VSTAB_INTERP_BILINEAR, dout, oh, ow, d_img,
                                         accumulate, d_theta, workspace, workspace_bytes, stream);
}

extern "C" int vstab_st_transform_interp_backward(const float *img, int B, int H, int W, int C, const float *theta, int theta_dim, int interp,
                                                  const float *dout, int oh, int ow, float *d_img, int accumulate, float *d_theta,
                                                  void *workspace, size_t workspace_bytes, void *stream)
{
    return st_transform_backward_checked("st_transform_interp_backward", img, B, H, W, C, theta, theta_dim, interp, dout, oh, ow, d_img,
                                         accumulate, d_theta, workspace, workspace_bytes, stream);
}

static int st_interp_backward_checked(const char *name, int interp, const float *img, int B, int H, int W, int C, const float *x, const float *y,
                                      const float *dout, int oh, int ow, float *d_img, int accumulate, float *d_x, float *d_y, void *stream)
{
    if (!img || !x || !y || !dout) return fail(nullptr, VSTAB_E_STATE, "%s: NULL buffer", name);
    if (!stx_shape_ok(B, H, W, C, oh, ow) || (long long)B * H * W * C > 0x7fffffffLL)
        return fail(nullptr, VSTAB_E_SHAPE, "%s: bad shape (B <= 65535)", name);
    if (!d_img && !d_x && !d_y) return fail(nullptr, VSTAB_E_SHAPE, "%s: d_img, d_x and d_y are all NULL", name);
    HIP_TRY(nullptr, launch_st_interp_backward(img, B, H, W, C, x, y, dout, oh, ow, d_img, accumulate ? 1 : 0, d_x, d_y, (hipStream_t)stream, interp));
    return VSTAB_OK;
}

extern "C" int vstab_st_bilinear_interp_backward(const float *img, int B, int H, int W, int C, const float *x, const float *y,
                                                 const float *dout, int oh, int ow, float *d_img, int accumulate, float *d_x, float *d_y,
                                                 void *stream)
{
    return st_interp_backward_checked("st_bilinear_interp_backward", VSTAB_INTERP_BILINEAR, img, B, H, W, C, x, y, dout, oh, ow, d_img, accumulate,
                                      d_x, d_y, stream);
}

extern "C" int vstab_st_bicubic_interp_backward(const float *img, int B, int H, int W, int C, const float *x, const float *y,
                                                const float *dout, int oh, int ow, float *d_img, int accumulate, float *d_x, float *d_y,
                                                void *stream)
{
    return st_interp_backward_checked("st_bicubic_interp_backward", VSTAB_INTERP_BICUBIC, img, B, H, W, C, x, y, dout, oh, ow, d_img, accumulate,
                                      d_x, d_y, stream);
}

// ---- ElasticTransformer: the coordinates the forward samples at, and the backward of its bilinear sampler
static bool tps_g_ok(int g) { return g >= 2 && g <= VSTAB_TPS_GMAX; }

extern "C" int vstab_st_elastic_coords(const float *theta, int B, int g, const float *linv_t, int oh, int ow, float *x_out, float *y_out,
                                       void *stream)
{
    if (!theta || !linv_t || !x_out || !y_out) return fail(nullptr, VSTAB_E_STATE, "st_elastic_coords: NULL buffer");
    if (!stx_shape_ok(B, 1, 1, 1, oh, ow) || !tps_g_ok(g))
        return fail(nullptr, VSTAB_E_SHAPE, "st_elastic_coords: bad shape (B <= 65535, grid side must be in [2, %d])", VSTAB_TPS_GMAX);
    HIP_TRY(nullptr, launch_st_elastic_coords(theta, B, g, linv_t, oh, ow, x_out, y_out, (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" size_t vstab_st_elastic_transform_backward_workspace_bytes(int B, int H, int W, int C, int g, int oh, int ow)
{
    if (!stx_shape_ok(B, H, W, C, oh, ow) || !tps_g_ok(g)) return 0;
    return st_elastic_backward_ws_bytes(B, H, W, C, g, oh, ow);
}

static int st_elastic_backward_checked(const char *name, const float *img, int B, int H, int W, int C, const float *theta, int g,
                                       const float *linv_t, int interp, const float *dout, int oh, int ow, float *d_img, int accumulate,
                                       float *d_theta, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!img || !theta || !linv_t || !dout) return fail(nullptr, VSTAB_E_STATE, "%s: NULL buffer", name);
    if (!stx_shape_ok(B, H, W, C, oh, ow) || (long long)B * H * W * C > 0x7fffffffLL || !tps_g_ok(g))
        return fail(nullptr, VSTAB_E_SHAPE, "%s: bad shape (B <= 65535, grid side must be in [2, %d])", name, VSTAB_TPS_GMAX);
    if (!interp_ok(interp)) return fail(nullptr, VSTAB_E_SHAPE, "%s: unknown interp %d", name, interp);
    if (!d_img && !d_theta) return fail(nullptr, VSTAB_E_SHAPE, "%s: d_img and d_theta are both NULL", name);
    if (d_theta) {
        const size_t need = st_elastic_backward_ws_bytes(B, H, W, C, g, oh, ow);
        if (!workspace || workspace_bytes < need) return fail(nullptr, VSTAB_E_NOMEM, "%s: workspace needs %zu bytes", name, need);
        if ((uintptr_t)workspace & 7) return fail(nullptr, VSTAB_E_ALIGN, "%s: workspace must be 8-byte aligned", name);
    }
    HIP_TRY(nullptr, launch_st_elastic_transform_backward(img, B, H, W, C, theta, g, linv_t, dout, oh, ow, d_img, accumulate ? 1 : 0, d_theta,
                                                          (double *)workspace, (hipStream_t)stream, interp));
    return VSTAB_OK;
}

extern "C" int vstab_st_elastic_transform_backward(const float *img, int B, int H, int W, int C, const float *theta, int g, const float *linv_t,
                                                   const float *dout, int oh, int ow, float *d_img, int accumulate, float *d_theta,
                                                   void *workspace, size_t workspace_bytes, void *stream)
{
    return st_elastic_backward_checked("st_elastic_transform_backward", img, B, H, W, C, theta, g, linv_t, VSTAB_INTERP_BILINEAR, dout, oh, ow,
                                       d_img, accumulate, d_theta, workspace, workspace_bytes, stream);
}

extern "C" int vstab_st_elastic_transform_interp_backward(const float *img, int B, int H, int W, int C, const float *theta, int g,
                                                          const float *linv_t, int interp, const float *dout, int oh, int ow, float *d_img,
                                                          int accumulate, float *d_theta, void *workspace, size_t workspace_bytes, void *stream)
{
    return st_elastic_backward_checked("st_elastic_transform_interp_backward", img, B, H, W, C, theta, g, linv_t, interp, dout, oh, ow, d_img,
                                       accumulate, d_theta, workspace, workspace_bytes, stream);
}

// ---- the symmetric-pad transformers: the matrices and coordinates the forward uses, and the backward of their bilinear sampler
static bool sym_kind_ok(int kind) { return kind == VSTAB_SYM_AFFINE || kind == VSTAB_SYM_PROJECTIVE || kind == VSTAB_SYM_SIMILARITY; }

// the forward's shape rule (vstab_st_symmetry_transform)
static bool sym_shape_ok(int B, int H, int W, int C, int oh, int ow)
{
    return oh >= 1 && ow >= 1 && oh <= (1 << 20) && ow <= (1 << 20) && stx_shape_ok(B, H, W, C, oh + 200, ow + 200);
}

extern "C" int vstab_st_symmetry_matrix(const float *theta, int B, int kind, float *out, void *stream)
{
    if (!theta || !out) return fail(nullptr, VSTAB_E_STATE, "st_symmetry_matrix: NULL buffer");
    if (B < 1 || B > 65535) return fail(nullptr, VSTAB_E_SHAPE, "st_symmetry_matrix: bad shape (1 <= B <= 65535)");
    if (!sym_kind_ok(kind)) return fail(nullptr, VSTAB_E_SHAPE, "st_symmetry_matrix: unknown kind %d", kind);
    HIP_TRY(nullptr, launch_st_symmetry_matrix(theta, B, kind, out, (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" int vstab_st_symmetry_coords(const float *theta, int B, int kind, int oh, int ow, float *x_out, float *y_out, void *stream)
{
    if (!theta || !x_out || !y_out) return fail(nullptr, VSTAB_E_STATE, "st_symmetry_coords: NULL buffer");
    if (!sym_shape_ok(B, 1, 1, 1, oh, ow)) return fail(nullptr, VSTAB_E_SHAPE, "st_symmetry_coords: bad shape (B <= 65535)");
    if (!sym_kind_ok(kind)) return fail(nullptr, VSTAB_E_SHAPE, "st_symmetry_coords: unknown kind %d", kind);
    HIP_TRY(nullptr, launch_st_symmetry_coords(theta, B, kind, oh, ow, x_out, y_out, (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" size_t vstab_st_symmetry_transform_backward_workspace_bytes(int B, int H, int W, int C, int oh, int ow)
{
    if (!sym_shape_ok(B, H, W, C, oh, ow) || H < 100 || W < 100) return 0;
    return st_symmetry_backward_ws_bytes(B, H, W, C, oh, ow);
}

static int st_symmetry_backward_checked(const char *name, const float *img, int B, int H, int W, int C, const float *theta, int kind, int interp,
                                        const float *dout, int oh, int ow, float *d_img, int accumulate, float *d_theta, void *workspace,
                                        size_t workspace_bytes, void *stream)
{
    if (!img || !theta || !dout) return fail(nullptr, VSTAB_E_STATE, "%s: NULL buffer", name);
    if (!sym_shape_ok(B, H, W, C, oh, ow) || (long long)B * H * W * C > 0x7fffffffLL)
        return fail(nullptr, VSTAB_E_SHAPE, "%s: bad shape (B <= 65535)", name);
    if (H < 100 || W < 100)
        return fail(nullptr, VSTAB_E_SHAPE, "%s: the 100-pixel symmetric pad needs H, W >= 100 (got %dx%d)", name, H, W);
    if (!sym_kind_ok(kind)) return fail(nullptr, VSTAB_E_SHAPE, "%s: unknown kind %d", name, kind);
    if (!interp_ok(interp)) return fail(nullptr, VSTAB_E_SHAPE, "%s: unknown interp %d", name, interp);
    if (!d_img && !d_theta) return fail(nullptr, VSTAB_E_SHAPE, "%s: d_img and d_theta are both NULL", name);
    if (d_theta) {
        const size_t need = st_symmetry_backward_ws_bytes(B, H, W, C, oh, ow);
        if (!workspace || workspace_bytes < need) return fail(nullptr, VSTAB_E_NOMEM, "%s: workspace needs %zu bytes", name, need);
        if ((uintptr_t)workspace & 7) return fail(nullptr, VSTAB_E_ALIGN, "%s: workspace must be 8-byte aligned", name);
    }
    HIP_TRY(nullptr, launch_st_symmetry_transform_backward(img, B, H, W, C, theta, kind, dout, oh, ow, d_img, accumulate ? 1 : 0, d_theta,
                                                           (double *)workspace, (hipStream_t)stream, interp));
    return VSTAB_OK;
}

extern "C" int vstab_st_symmetry_transform_backward(const float *img, int B, int H, int W, int C, const float *theta, int kind, const float *dout,
                                                    int oh, int ow, float *d_img, int accumulate, float *d_theta, void *workspace,
                                                    size_t workspace_bytes, void *stream)
{
    return st_symmetry_backward_checked("st_symmetry_transform_backward", img, B, H, W, C, theta, kind, VSTAB_INTERP_BILINEAR, dout, oh, ow, d_img,
                                        accumulate, d_theta, workspace, workspace_bytes, stream);
}

extern "C" int vstab_st_symmetry_transform_interp_backward(const float *img, int B, int H, int W, int C, const float *theta, int kind, int interp,
                                                           const float *dout, int oh, int ow, float *d_img, int accumulate, float *d_theta,
                                                           void *workspace, size_t workspace_bytes, void *stream)
{
    return st_symmetry_backward_checked("st_symmetry_transform_interp_backward", img, B, H, W, C, theta, kind, interp, dout, oh, ow, d_img,
                                        accumulate, d_theta, workspace, workspace_bytes, stream);
}

// ---- the 3-D volume transformer (sampler3d_ops.hip).  The shape is judged before the pointers: a shape outside the contract is
// VSTAB_E_SHAPE whatever else is wrong with the call.
static bool st3d_shape_ok(int B, int D, int H, int W, int C, int od, int oh, int ow, int edge)
{
    const long long lim = 1ll << 24, cap = 1ll << 40;          // fp32 holds every padded index; element counts far inside 63 bits
    if (B < 1 || B > 65535 || D < 1 || H < 1 || W < 1 || C < 1 || od < 1 || oh < 1 || ow < 1 || edge < 0 || edge > (1 << 22)) return false;
    if (D + 2ll * edge > lim || H + 2ll * edge > lim || W + 2ll * edge > lim || od > lim || oh > lim || ow > lim || C > lim) return false;
    const long long vin = (long long)D * H, vout = (long long)od * oh;                   // < 2^48 each
    if (vin > cap / W || vout > cap / ow) return false;
    if (vin * W > cap / C / B || vout * ow > cap / C / B) return false;
    int nbx, nby, nbz;
    long long bricks;
    return st3d_plan(B, od, oh, ow, nbx, nby, nbz, bricks);
}

extern "C" int vstab_st3d_meshgrid(float *out, int od, int oh, int ow, void *stream)
{
    if (od < 1 || oh < 1 || ow < 1 || od > (1 << 24) || oh > (1 << 24) || ow > (1 << 24) || (long long)od * oh > (1ll << 38) / ow)
        return fail(nullptr, VSTAB_E_SHAPE, "st3d_meshgrid: bad shape (at most 2^38 voxels)");
    if (!out) return fail(nullptr, VSTAB_E_STATE, "st3d_meshgrid: NULL buffer");
    HIP_TRY(nullptr, launch_st3d_meshgrid(out, od, oh, ow, (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" int vstab_st3d_bilinear_interp(const float *vol, int B, int D, int H, int W, int C, const float *x, const float *y, const float *z,
                                          int od, int oh, int ow, int edge_size, float *out, void *stream)
{
    if (!st3d_shape_ok(B, D, H, W, C, od, oh, ow, edge_size)) return fail(nullptr, VSTAB_E_SHAPE, "st3d_bilinear_interp: bad shape (edge_size >= 0, B <= 65535)");
    if (!vol || !x || !y || !z || !out) return fail(nullptr, VSTAB_E_STATE, "st3d_bilinear_interp: NULL buffer");
    HIP_TRY(nullptr, launch_st3d_interp(vol, B, D, H, W, C, x, y, z, od, oh, ow, edge_size, out, (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" int vstab_st3d_transform(const float *vol, int B, int D, int H, int W, int C, const float *theta, float *out, int od, int oh, int ow,
                                    void *stream)
{
    if (!st3d_shape_ok(B, D, H, W, C, od, oh, ow, 1)) return fail(nullptr, VSTAB_E_SHAPE, "st3d_transform: bad shape (B <= 65535)");
    if (!vol || !theta || !out) return fail(nullptr, VSTAB_E_STATE, "st3d_transform: NULL buffer");
    HIP_TRY(nullptr, launch_st3d_transform(vol, B, D, H, W, C, theta, out, od, oh, ow, (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" size_t vstab_st3d_transform_backward_workspace_bytes(int B, int D, int H, int W, int C, int od, int oh, int ow)
{
    if (!st3d_shape_ok(B, D, H, W, C, od, oh, ow, 1)) return 0;
    return st3d_transform_backward_ws_bytes(B, od, oh, ow);
}

extern "C" int vstab_st3d_transform_backward(const float *vol, int B, int D, int H, int W, int C, const float *theta, const float *dout, int od,
                                             int oh, int ow, float *d_vol, int accumulate, float *d_theta, void *workspace,
                                             size_t workspace_bytes, void *stream)
{
    if (!st3d_shape_ok(B, D, H, W, C, od, oh, ow, 1)) return fail(nullptr, VSTAB_E_SHAPE, "st3d_transform_backward: bad shape (B <= 65535)");
    if (!vol || !theta || !dout) return fail(nullptr, VSTAB_E_STATE, "st3d_transform_backward: NULL buffer");
    if (!d_vol && !d_theta) return fail(nullptr, VSTAB_E_SHAPE, "st3d_transform_backward: d_vol and d_theta are both NULL");
    if (d_theta) {
        const size_t need = st3d_transform_backward_ws_bytes(B, od, oh, ow);
        if (!workspace || workspace_bytes < need) return fail(nullptr, VSTAB_E_NOMEM, "st3d_transform_backward: workspace needs %zu bytes", need);
        if ((uintptr_t)workspace & 7) return fail(nullptr, VSTAB_E_ALIGN, "st3d_transform_backward: workspace must be 8-byte aligned");
    }
    HIP_TRY(nullptr, launch_st3d_transform_backward(vol, B, D, H, W, C, theta, dout, od, oh, ow, d_vol, accumulate ? 1 : 0, d_theta,
                                                    (double *)workspace, (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" int vstab_st3d_bilinear_interp_backward(const float *vol, int B, int D, int H, int W, int C, const float *x, const float *y,
                                                   const float *z, int od, int oh, int ow, int edge_size, const float *dout, float *d_vol,
                                                   int accumulate, float *dx, float *dy, float *dz, void *stream)
{
    if (!st3d_shape_ok(B, D, H, W, C, od, oh, ow, edge_size))
        return fail(nullptr, VSTAB_E_SHAPE, "st3d_bilinear_interp_backward: bad shape (edge_size >= 0, B <= 65535)");
    if (!vol || !x || !y || !z || !dout) return fail(nullptr, VSTAB_E_STATE, "st3d_bilinear_interp_backward: NULL buffer");
    if (!d_vol && !dx && !dy && !dz) return fail(nullptr, VSTAB_E_SHAPE, "st3d_bilinear_interp_backward: d_vol, dx, dy and dz are all NULL");
    HIP_TRY(nullptr, launch_st3d_interp_backward(vol, B, D, H, W, C, x, y, z, od, oh, ow, edge_size, dout, d_vol, accumulate ? 1 : 0, dx, dy, dz,
                                                 (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" int vstab_vec2mtrx(const float *p, int B, int dim, int warp_approx, float *out, void *stream)
{
    if (!p || !out) return fail(nullptr, VSTAB_E_STATE, "vec2mtrx: NULL buffer");
    if (B < 1 || (dim != 8 && dim != 6) || warp_approx < 1 || warp_approx > 64)
        return fail(nullptr, VSTAB_E_SHAPE, "vec2mtrx: p must be [B,8] or [B,6], 1 <= warpApprox <= 64");
    HIP_TRY(nullptr, launch_vec2mtrx(p, B, dim, warp_approx, out, (hipStream_t)stream));
    return VSTAB_OK;
}

// ---- backward of warp.py's samplers (sampler_ops.hip): conventions of vstab_st_transform_backward
extern "C" size_t vstab_homography_warp_backward_workspace_bytes(int B, int Hi, int Wi, int C, int oh, int ow)
{
    if (!stx_shape_ok(B, Hi, Wi, C, oh, ow)) return 0;
    return homography_warp_backward_ws_bytes(B, Hi, Wi, C, oh, ow);
}

// `ref` null: vstab_homography_warp_backward (mat = M), else vstab_transform_image_backward (mat = pM)
static int homography_backward(const char *who, const float *img, int B, int Hi, int Wi, int C, const float *mat, const float *ref,
                               const float *dout, int oh, int ow, float *d_img, int accumulate, float *d_mat, void *workspace,
                               size_t workspace_bytes, void *stream)
{
    if (!stx_shape_ok(B, Hi, Wi, C, oh, ow) || (long long)B * Hi * Wi * C > 0x7fffffffLL)
        return fail(nullptr, VSTAB_E_SHAPE, "%s: bad shape (B <= 65535, B*Hi*Wi*C < 2^31)", who);
    if (!d_img && !d_mat) return fail(nullptr, VSTAB_E_SHAPE, "%s: d_img and the matrix gradient are both NULL", who);
    if (d_mat) {
        const size_t need = homography_warp_backward_ws_bytes(B, Hi, Wi, C, oh, ow);
        if (!workspace || workspace_bytes < need) return fail(nullptr, VSTAB_E_NOMEM, "%s: workspace needs %zu bytes", who, need);
        if ((uintptr_t)workspace & 7) return fail(nullptr, VSTAB_E_ALIGN, "%s: workspace must be 8-byte aligned", who);
    }
    HIP_TRY(nullptr, launch_homography_warp_backward(img, B, Hi, Wi, C, mat, ref, dout, oh, ow, d_img, accumulate ? 1 : 0, d_mat,
                                                     (double *)workspace, (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" int vstab_homography_warp_backward(const float *img, int B, int Hi, int Wi, int C, const float *M, const float *dout, int oh, int ow,
                                              float *d_img, int accumulate, float *d_M, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!img || !M || !dout) return fail(nullptr, VSTAB_E_STATE, "homography_warp_backward: NULL buffer");
    return homography_backward("homography_warp_backward", img, B, Hi, Wi, C, M, nullptr, dout, oh, ow, d_img, accumulate, d_M, workspace,
                               workspace_bytes, stream);
}

extern "C" int vstab_transform_image_backward(const float *img, int B, int Hi, int Wi, int C, const float *ref, const float *pM, const float *dout,
                                              int oh, int ow, float *d_img, int accumulate, float *d_pM, void *workspace, size_t workspace_bytes,
                                              void *stream)
{
    if (!img || !ref || !pM || !dout) return fail(nullptr, VSTAB_E_STATE, "transform_image_backward: NULL buffer");
    return homography_backward("transform_image_backward", img, B, Hi, Wi, C, pM, ref, dout, oh, ow, d_img, accumulate, d_pM, workspace,
                               workspace_bytes, stream);
}

extern "C" int vstab_vec2mtrx_backward(const float *p, int B, int dim, int warp_approx, const float *d_out, float *d_p, void *stream)
{
    if (!p || !d_out || !d_p) return fail(nullptr, VSTAB_E_STATE, "vec2mtrx_backward: NULL buffer");
    if (B < 1 || (dim != 8 && dim != 6) || warp_approx < 1 || warp_approx > 64)
        return fail(nullptr, VSTAB_E_SHAPE, "vec2mtrx_backward: p must be [B,8] or [B,6], 1 <= warpApprox <= 64");
    HIP_TRY(nullptr, launch_vec2mtrx_backward(p, B, dim, warp_approx, d_out, d_p, (hipStream_t)stream));
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
