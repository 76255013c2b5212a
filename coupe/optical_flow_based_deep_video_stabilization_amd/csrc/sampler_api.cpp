// C ABI of the samplers (include/vstab.h): spatial_transformer.py's 2-D transformers (sampler_ops.hip), the 3-D volume transformer
// (sampler3d_ops.hip) and warp.py's homography warp and matrix exponential, forward and backward.  Every entry point is its checks, in
// the order the tests pin (tests/test_sampler_abi_refusals_cpu.py), and one launch.  A `foo` / `foo_interp` pair is two exported
// symbols over one checked function that takes the name of the one called.
#include <cmath>
#include <vector>

#include "api_internal.h"

using namespace vstab;

// ------------------------------------------------------------------------- the rules the entry points share
static bool interp_ok(int interp) { return interp == VSTAB_INTERP_BILINEAR || interp == VSTAB_INTERP_BICUBIC; }

static bool tps_g_ok(int g) { return g >= 2 && g <= VSTAB_TPS_GMAX; }

static bool sym_kind_ok(int kind) { return kind == VSTAB_SYM_AFFINE || kind == VSTAB_SYM_PROJECTIVE || kind == VSTAB_SYM_SIMILARITY; }

static bool stx_shape_ok(int B, int H, int W, int C, int oh, int ow)
{
    return B >= 1 && B <= 65535 && H >= 1 && W >= 1 && C >= 1 && oh >= 1 && ow >= 1 && (long long)oh * ow <= 0x7fffffffLL / 4 &&
           (long long)H * W <= 0x7fffffffLL;
}

// the symmetric-pad transformers sample (oh+200) x (ow+200) points; tf.pad SYMMETRIC of 100 px needs H, W >= 100 on top (judged
// apart: it has a message of its own)
static bool sym_shape_ok(int B, int H, int W, int C, int oh, int ow)
{
    return oh >= 1 && ow >= 1 && oh <= (1 << 20) && ow <= (1 << 20) && stx_shape_ok(B, H, W, C, oh + 200, ow + 200);
}

// the backwards index the input with 32 bits
static bool fits_i32(int B, int H, int W, int C) { return (long long)B * H * W * C <= 0x7fffffffLL; }

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

// The gradient contract of every backward with a parameter gradient: the caller asks for the input's gradient (d_in), the
// parameters' (d_par), or both -- `pair` names the two in the entry's words; d_par is summed in two stages through a workspace of
// `need` bytes (the launcher's *_ws_bytes; not asked for without d_par), 8-byte aligned because it holds doubles.  VSTAB_OK, or the refusal.
static int grad_outputs_checked(const char *name, const char *pair, const void *d_in, const void *d_par, size_t need, const void *workspace,
                                size_t workspace_bytes)
{
    if (!d_in && !d_par) return fail(nullptr, VSTAB_E_SHAPE, "%s: %s are both NULL", name, pair);
    if (d_par) {
        if (!workspace || workspace_bytes < need) return fail(nullptr, VSTAB_E_NOMEM, "%s: workspace needs %zu bytes", name, need);
        if ((uintptr_t)workspace & 7) return fail(nullptr, VSTAB_E_ALIGN, "%s: workspace must be 8-byte aligned", name);
    }
    return VSTAB_OK;
}

// ------------------------------------------------------------------------- AffineTransformer / ProjectiveTransformer, the plain samplers
extern "C" int vstab_st_transform(const float *img, int B, int H, int W, int C, const float *theta, int theta_dim,
                                  float *out, int oh, int ow, void *stream)
{
    if (!img || !theta || !out) return fail(nullptr, VSTAB_E_STATE, "st_transform: NULL buffer");
    if (B < 1 || H < 1 || W < 1 || C < 1 || oh < 1 || ow < 1 || (theta_dim != 6 && theta_dim != 8))
        return fail(nullptr, VSTAB_E_SHAPE, "st_transform: bad shape (theta must be [B,6] or [B,8])");
    HIP_TRY(nullptr, launch_st_transform(img, B, H, W, C, theta, theta_dim, out, oh, ow, (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" int vstab_st_transform_interp(const float *img, int B, int H, int W, int C, const float *theta, int theta_dim, int interp,
                                         float *out, int oh, int ow, void *stream)
{
    if (!img || !theta || !out) return fail(nullptr, VSTAB_E_STATE, "st_transform_interp: NULL buffer");
    if (!stx_shape_ok(B, H, W, C, oh, ow) || (theta_dim != 6 && theta_dim != 8))
        return fail(nullptr, VSTAB_E_SHAPE, "st_transform_interp: bad shape (theta must be [B,6] or [B,8])");
    if (!interp_ok(interp)) return fail(nullptr, VSTAB_E_SHAPE, "st_transform_interp: unknown interp %d", interp);
    HIP_TRY(nullptr, launch_st_transform_interp(img, B, H, W, C, theta, theta_dim, interp, out, oh, ow, (hipStream_t)stream));
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

extern "C" int vstab_st_bicubic_interp(const float *img, int B, int H, int W, int C, const float *x, const float *y, int oh, int ow,
                                       float *out, void *stream)
{
    if (!img || !x || !y || !out) return fail(nullptr, VSTAB_E_STATE, "st_bicubic_interp: NULL buffer");
    if (!stx_shape_ok(B, H, W, C, oh, ow)) return fail(nullptr, VSTAB_E_SHAPE, "st_bicubic_interp: bad shape");
    HIP_TRY(nullptr, launch_st_bicubic_interp(img, B, H, W, C, x, y, oh, ow, out, (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" int vstab_st_meshgrid(float *out, int oh, int ow, void *stream)
{
    if (!out) return fail(nullptr, VSTAB_E_STATE, "st_meshgrid: NULL buffer");
    if (oh < 1 || ow < 1 || (long long)oh * ow > 0x7fffffffLL / 3) return fail(nullptr, VSTAB_E_SHAPE, "st_meshgrid: bad shape");
    HIP_TRY(nullptr, launch_st_meshgrid(out, oh, ow, (hipStream_t)stream));
    return VSTAB_OK;
}

// ---- their backward: d img by float atomics, d theta by a reproducible two-stage sum
extern "C" size_t vstab_st_transform_backward_workspace_bytes(int B, int H, int W, int C, int oh, int ow)
{
    if (!stx_shape_ok(B, H, W, C, oh, ow)) return 0;
    return st_transform_backward_ws_bytes(B, H, W, C, oh, ow);
}

static int st_transform_backward_checked(const char *name, const float *img, int B, int H, int W, int C, const float *theta, int theta_dim,
                                         int interp, const float *dout, int oh, int ow, float *d_img, int accumulate, float *d_theta,
                                         void *workspace, size_t workspace_bytes, void *stream)
{
    if (!img || !theta || !dout) return fail(nullptr, VSTAB_E_STATE, "%s: NULL buffer", name);
    if (!stx_shape_ok(B, H, W, C, oh, ow) || !fits_i32(B, H, W, C) || (theta_dim != 6 && theta_dim != 8))
        return fail(nullptr, VSTAB_E_SHAPE, "%s: bad shape (theta must be [B,6] or [B,8], B <= 65535)", name);
    if (!interp_ok(interp)) return fail(nullptr, VSTAB_E_SHAPE, "%s: unknown interp %d", name, interp);
    if (const int rc = grad_outputs_checked(name, "d_img and d_theta", d_img, d_theta, d_theta ? st_transform_backward_ws_bytes(B, H, W, C, oh, ow) : 0,
                                            workspace, workspace_bytes))
        return rc;
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
    if (!stx_shape_ok(B, H, W, C, oh, ow) || !fits_i32(B, H, W, C)) return fail(nullptr, VSTAB_E_SHAPE, "%s: bad shape (B <= 65535)", name);
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

// ------------------------------------------------------------------------- the symmetric-pad transformers
extern "C" int vstab_st_symmetry_transform(const float *img, int B, int H, int W, int C, const float *theta, int kind, int interp,
                                           float *out, int oh, int ow, void *stream)
{
    if (!img || !theta || !out) return fail(nullptr, VSTAB_E_STATE, "st_symmetry_transform: NULL buffer");
    if (!sym_shape_ok(B, H, W, C, oh, ow)) return fail(nullptr, VSTAB_E_SHAPE, "st_symmetry_transform: bad shape");
    if (H < 100 || W < 100)
        return fail(nullptr, VSTAB_E_SHAPE, "st_symmetry_transform: the 100-pixel symmetric pad needs H, W >= 100 (got %dx%d)", H, W);
    if (!sym_kind_ok(kind)) return fail(nullptr, VSTAB_E_SHAPE, "st_symmetry_transform: unknown kind %d", kind);
    if (!interp_ok(interp)) return fail(nullptr, VSTAB_E_SHAPE, "st_symmetry_transform: unknown interp %d", interp);
    HIP_TRY(nullptr, launch_st_symmetry_transform(img, B, H, W, C, theta, kind, interp, out, oh, ow, (hipStream_t)stream));
    return VSTAB_OK;
}

// the matrices and coordinates the forward uses
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
    if (!sym_shape_ok(B, H, W, C, oh, ow) || !fits_i32(B, H, W, C)) return fail(nullptr, VSTAB_E_SHAPE, "%s: bad shape (B <= 65535)", name);
    if (H < 100 || W < 100)
        return fail(nullptr, VSTAB_E_SHAPE, "%s: the 100-pixel symmetric pad needs H, W >= 100 (got %dx%d)", name, H, W);
    if (!sym_kind_ok(kind)) return fail(nullptr, VSTAB_E_SHAPE, "%s: unknown kind %d", name, kind);
    if (!interp_ok(interp)) return fail(nullptr, VSTAB_E_SHAPE, "%s: unknown interp %d", name, interp);
    if (const int rc = grad_outputs_checked(name, "d_img and d_theta", d_img, d_theta, d_theta ? st_symmetry_backward_ws_bytes(B, H, W, C, oh, ow) : 0,
                                            workspace, workspace_bytes))
        return rc;
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

// ------------------------------------------------------------------------- ElasticTransformer (thin-plate spline)
// ElasticTransformer._initialize_tps (ST:187-225) in double: L (K+3)x(K+3) from the fp32 linspace control points, inverted by
// Gauss-Jordan with partial pivoting, transpose(L_inv[:,3:]) rounded to fp32 into linv_t [K, K+3]
extern "C" int vstab_host_tps_linv(int g, float *linv_t, int cap)
{
    if (!linv_t) return fail(nullptr, VSTAB_E_STATE, "host_tps_linv: linv_t is NULL");
    if (!tps_g_ok(g)) return fail(nullptr, VSTAB_E_SHAPE, "host_tps_linv: grid side %d outside [2, %d] (g = 1 makes L singular)", g, VSTAB_TPS_GMAX);
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
    if (!stx_shape_ok(B, H, W, C, oh, ow) || !tps_g_ok(g))
        return fail(nullptr, VSTAB_E_SHAPE, "st_elastic_transform: bad shape (grid side must be in [2, %d])", VSTAB_TPS_GMAX);
    if (!interp_ok(interp)) return fail(nullptr, VSTAB_E_SHAPE, "st_elastic_transform: unknown interp %d", interp);
    HIP_TRY(nullptr, launch_st_elastic_transform(img, B, H, W, C, theta, g, linv_t, interp, out, oh, ow, (hipStream_t)stream));
    return VSTAB_OK;
}

// the coordinates the forward samples at
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
    if (!stx_shape_ok(B, H, W, C, oh, ow) || !fits_i32(B, H, W, C) || !tps_g_ok(g))
        return fail(nullptr, VSTAB_E_SHAPE, "%s: bad shape (B <= 65535, grid side must be in [2, %d])", name, VSTAB_TPS_GMAX);
    if (!interp_ok(interp)) return fail(nullptr, VSTAB_E_SHAPE, "%s: unknown interp %d", name, interp);
    if (const int rc = grad_outputs_checked(name, "d_img and d_theta", d_img, d_theta, d_theta ? st_elastic_backward_ws_bytes(B, H, W, C, g, oh, ow) : 0,
                                            workspace, workspace_bytes))
        return rc;
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

// ------------------------------------------------------------------------- the 3-D volume transformer (sampler3d_ops.hip)
// The shape is judged before the pointers: a shape outside the contract is VSTAB_E_SHAPE whatever else is wrong with the call.
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
    if (const int rc = grad_outputs_checked("st3d_transform_backward", "d_vol and d_theta", d_vol, d_theta,
                                            d_theta ? st3d_transform_backward_ws_bytes(B, od, oh, ow) : 0, workspace, workspace_bytes))
        return rc;
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

// ------------------------------------------------------------------------- warp.py: the homography warp and the matrix exponential
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

extern "C" int vstab_vec2mtrx(const float *p, int B, int dim, int warp_approx, float *out, void *stream)
{
    if (!p || !out) return fail(nullptr, VSTAB_E_STATE, "vec2mtrx: NULL buffer");
    if (B < 1 || (dim != 8 && dim != 6) || warp_approx < 1 || warp_approx > 64)
        return fail(nullptr, VSTAB_E_SHAPE, "vec2mtrx: p must be [B,8] or [B,6], 1 <= warpApprox <= 64");
    HIP_TRY(nullptr, launch_vec2mtrx(p, B, dim, warp_approx, out, (hipStream_t)stream));
    return VSTAB_OK;
}

// ---- their backward: conventions of vstab_st_transform_backward
extern "C" size_t vstab_homography_warp_backward_workspace_bytes(int B, int Hi, int Wi, int C, int oh, int ow)
{
    if (!stx_shape_ok(B, Hi, Wi, C, oh, ow)) return 0;
    return homography_warp_backward_ws_bytes(B, Hi, Wi, C, oh, ow);
}

// `ref` null: vstab_homography_warp_backward (mat = M), else vstab_transform_image_backward (mat = pM); either has judged its pointers
static int homography_backward(const char *who, const float *img, int B, int Hi, int Wi, int C, const float *mat, const float *ref,
                               const float *dout, int oh, int ow, float *d_img, int accumulate, float *d_mat, void *workspace,
                               size_t workspace_bytes, void *stream)
{
    if (!stx_shape_ok(B, Hi, Wi, C, oh, ow) || !fits_i32(B, Hi, Wi, C))
        return fail(nullptr, VSTAB_E_SHAPE, "%s: bad shape (B <= 65535, B*Hi*Wi*C < 2^31)", who);
    if (const int rc = grad_outputs_checked(who, "d_img and the matrix gradient", d_img, d_mat,
                                            d_mat ? homography_warp_backward_ws_bytes(B, Hi, Wi, C, oh, ow) : 0, workspace, workspace_bytes))
        return rc;
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
