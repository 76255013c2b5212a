// Samplers named by the reference's spatial_transformer.py and warp.py (BASELINE configs[2]'s
// "spatial_transformer warp").  HBM-bound tap gathers, coordinates generated in-kernel (no grid tensor is materialised).
// ONE family of kernels, templated on where a pixel's source coordinates come from (XS_*) and on the sampler (XI_*):
// st3_tile_kernel for 3-channel frames (tile3.h's skeleton: 2-D tiles, 3-dword tap gathers, rows leaving as 16-byte stores),
// st_pixel_kernel (one thread per pixel) for other channel counts.  Each piece of the reference's arithmetic is one device
// function (st_axis in st_axis.h, st_taps, homog_taps, st_blend, cubic_axis, st_coords) that both kernels call.  The bilinear sampler of the theta,
// explicit-coordinate, symmetric-pad and thin-plate-spline sources has a backward (st3_tile_bwd_kernel / st_pixel_bwd_kernel and, for the spline,
// st3_tile_tps_bwd_kernel / st_pixel_tps_bwd_kernel, at the end of the file) that calls the same functions; its d img is summed by
// float atomics and depends on their arrival order in its last bits, its d theta is reproducible.  The bicubic sampler of the same four
// sources has its backward in the same kernels (INTERP = XI_BICUBIC: st_cubic_bwd_point / st3_cubic_bwd_point).  The homography source has its own
// backward arithmetic (homog_bwd_point / homog3_bwd_point, d M [B,9]) on the same two kernel skeletons, and vec2mtrx its own kernel.
// -ffp-contract=off keeps the weight arithmetic the reference's op-by-op fp32 sequence.
#include "vstab_internal.h"
#include "hbm_profile.h"
#include "tile3.h"
#include "st_axis.h"
#include <algorithm>

namespace vstab {

// _meshgrid(out_size) (spatial_transformer.py:755-779): flat [3*oh*ow] = x_t row, y_t row, ones
__global__ __launch_bounds__(256) void st_meshgrid_kernel(float *__restrict__ out, int oh, int ow)
{
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const int np = oh * ow;
    if (idx >= np) return;
    const int oy = idx / ow, ox = idx - oy * ow;
    out[idx] = lin11(ox, ow);
    out[np + idx] = lin11(oy, oh);
    out[2 * np + idx] = 1.0f;
}

// M = refMtrx . pMtrx (warp.py:48-49's tf.matmul) composed here when `ref` is given: every product and sum its own fp32 operation,
// (r0*p0 + r1*p1) + r2*p2, like the grid products below -- no library GEMM in front of the launch
__device__ __forceinline__ void compose3(const float *__restrict__ ref, const float *__restrict__ p, float *m)
{
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) m[3 * i + j] = (ref[3 * i] * p[j] + ref[3 * i + 1] * p[3 + j]) + ref[3 * i + 2] * p[6 + j];
}

// ---------------------------------------------------------------------------------
// Where a pixel's source coordinates come from, and the sampler:
//   XS_COORDS  explicit x, y [B*oh*ow]                       (bilinear_interp ST:902-964, bicubic_interp ST:966-1072)
//   XS_THETA   Affine/ProjectiveTransformer.transform: T_g = theta . (x_t, y_t, 1) on the linspace(-1,1) grid of the OUTPUT size;
//              projective divides by z with z == 0 replaced by z + 1e-8 (ST:400-452, 539-608)
//   XS_SYM     the symmetric-pad transformers (SimilarityTransformer ST:311-371, AffineSymmetryTransformer ST:454-517,
//              ProjectiveSymmetryTransformer ST:611-716): the image padded by 100 px per side in SYMMETRIC mode is never
//              materialised (a padded index p reads refl(p - 100)); the (oh+200) x (ow+200) grid is sampled only where
//              resize_image_with_crop_or_pad keeps it, the pixels it pads are written as zeros
//   XS_TPS     ElasticTransformer's thin-plate spline (ST:40-224): coeff [2, K+3] = (source points + theta) . L_inv^T once per
//              workgroup into LDS, then per pixel x_s = coeff_x . [x_t, y_t, 1, U_1..U_K] with U_k = r^2 ln r^2 evaluated
//              in-kernel (no (K+1) x N table)
//   XS_HOMOG   warp.transformImage / transformCropImage (warp.py:46-129): homography from the canonical [-1,1]^2 grid
//              (np.linspace in float64, cast to fp32) straight to source PIXEL coordinates, /(z+1e-8), floor/ceil taps, taps
//              outside the image read an appended zero row.  M = refMtrx . pMtrx, row-major [B,9].  XI_BILINEAR only.
//   XI_BILINEAR  bilinear_interp: normalised coordinates in [-1,1] against an image zero-padded by one pixel (st_taps)
//   XI_BICUBIC   bicubic_interp: 16 taps, edges replicate (cubic_axis)
// ---------------------------------------------------------------------------------
enum { XS_THETA = 0, XS_COORDS = 1, XS_HOMOG = 2, XS_SYM = 3, XS_TPS = 4 };      // THETA = 0 and HOMOG = 2: the names bench.py reports
enum { XI_BILINEAR = 0, XI_BICUBIC = 1 };
constexpr int ST_TPS_KMAX = 256;                     // g <= 16 control points per side (api.cpp)

struct StSrc {
    const float *x, *y;            // XS_COORDS
    const float *theta;            // XS_THETA [B,tdim]; XS_SYM [B,6|8|4]; XS_TPS [B,2K]; XS_HOMOG M (or pMtrx) [B,9]
    const float *ref;              // XS_HOMOG: refMtrx (theta = pMtrx then) or null
    const float *linv_t;           // XS_TPS: transpose(L_inv[:,3:]) [K, K+3]
    int tdim, kind, g, B;          // kind: XS_SYM's VSTAB_SYM_* (0 affine, 1 projective, 2 similarity); g: TPS grid side
    int gh, gw;                    // the linspace sampling grid
    float sx, sy;                  // its steps 2/(n-1), divided once on the host (the same IEEE quotient lin11 computes): fp32 for
    double dsx, dsy;               // tf.linspace, fp64 for XS_HOMOG's np.linspace
    int pady, cropy, leny, padx, cropx, lenx;        // XS_SYM's crop-or-pad: final i reads grid i - pad + crop when 0 <= i - pad < len
};

// the four taps of one output pixel: image coordinates clamped into the image (what is addressed), validity per axis (what
// counts: an invalid tap reads as zero) and the blend weights (ST: w00, w01, w10, w11; homography: xr, yr)
struct Taps { int xa, xb, ya, yb; bool vxa, vxb, vya, vyb; float w0, w1, w2, w3; };

__device__ __forceinline__ Taps st_taps(const Axis &X, const Axis &Y)
{
    Taps t;
    t.w0 = X.hi * Y.hi; t.w1 = X.lo * Y.hi;
    t.w2 = X.hi * Y.lo; t.w3 = X.lo * Y.lo;
    t.vxa = X.va; t.vxb = X.vb; t.vya = Y.va; t.vyb = Y.vb;
    t.xa = X.a; t.xb = X.b; t.ya = Y.a; t.yb = Y.b;
    return t;
}

__device__ __forceinline__ Taps st_taps(float xn, float yn, int H, int W) { return st_taps(st_axis(xn, W), st_axis(yn, H)); }

// the homography at grid point (ox, oy): the grid values X, Y, the products before the division xh, yh, zs = zh + 1e-8f (which the
// backward's chain rule needs) and the source pixel coordinates xw, yw
struct HomogPt { float X, Y, xh, yh, zs, xw, yw; };

__device__ __forceinline__ HomogPt homog_coords(const float *__restrict__ m, int ox, int oy, double dsx, double dsy)
{
    HomogPt q;
    q.X = (float)(-1.0 + (double)ox * dsx);
    q.Y = (float)(-1.0 + (double)oy * dsy);
    q.xh = (m[0] * q.X + m[1] * q.Y) + m[2];
    q.yh = (m[3] * q.X + m[4] * q.Y) + m[5];
    const float zh = (m[6] * q.X + m[7] * q.Y) + m[8];
    q.zs = zh + 1e-8f;
    q.xw = q.xh / q.zs; q.yw = q.yh / q.zs;
    return q;
}

__device__ __forceinline__ Taps homog_taps(const HomogPt &q, int Hi, int Wi)
{
    const float xw = q.xw, yw = q.yw;
    const float xf = floorf(xw), xc = ceilf(xw), yf = floorf(yw), yc = ceilf(yw);
    // clamp before the int conversion (out-of-range float->int is undefined); anything outside is "outside"
    const float lim = 1.0e9f;
    const int xfi = (int)fminf(fmaxf(xf, -lim), lim), xci = (int)fminf(fmaxf(xc, -lim), lim);
    const int yfi = (int)fminf(fmaxf(yf, -lim), lim), yci = (int)fminf(fmaxf(yc, -lim), lim);
    Taps t;
    t.w0 = xw - xf; t.w1 = yw - yf; t.w2 = 0.f; t.w3 = 0.f;
    t.vxa = xfi >= 0 && xfi < Wi; t.vxb = xci >= 0 && xci < Wi; t.vya = yfi >= 0 && yfi < Hi; t.vyb = yci >= 0 && yci < Hi;
    t.xa = min(max(xfi, 0), Wi - 1); t.xb = min(max(xci, 0), Wi - 1);
    t.ya = min(max(yfi, 0), Hi - 1); t.yb = min(max(yci, 0), Hi - 1);
    return t;
}

__device__ __forceinline__ Taps homog_taps(const float *__restrict__ m, int ox, int oy, double dsx, double dsy, int Hi, int Wi)
{
    return homog_taps(homog_coords(m, ox, oy, dsx, dsy), Hi, Wi);
}

template <bool HOMOG>
__device__ __forceinline__ float st_blend(const Taps &t, float I00, float I01, float I10, float I11)
{
    if (HOMOG) {
        const float xr = t.w0, yr = t.w1;        // image*(1-Xratio)*(1-Yratio) evaluates left to right: (I*(1-xr))*(1-yr)
        return (((I00 * (1.0f - xr)) * (1.0f - yr) + (I01 * xr) * (1.0f - yr)) + (I10 * (1.0f - xr)) * yr) + (I11 * xr) * yr;
    }
    return ((t.w0 * I00 + t.w1 * I01) + t.w2 * I10) + t.w3 * I11;      // tf.add_n order
}

// np.pad(mode='symmetric') index map for one reflection (|u| stays within one image size: H, W >= 100 on the host)
__device__ __forceinline__ int refl(int u, int n) { return u < 0 ? -u - 1 : (u >= n ? 2 * n - 1 - u : u); }

// the sample's 2x3 / 3x3 matrix, theta pre-maps included, every product and sum its own fp32 operation
template <int SRC>
__device__ __forceinline__ void st_matrix(const StSrc &S, int n, float *th)
{
    if (SRC == XS_THETA || SRC == XS_HOMOG) {
        const float *tp = S.theta + (long long)n * S.tdim;       // wave-uniform: scalar loads
#pragma unroll
        for (int k = 0; k < 9; ++k) th[k] = k < S.tdim ? tp[k] : 1.0f;
        if (SRC == XS_HOMOG && S.ref) {                            // M = refMtrx . pMtrx, here instead of a GEMM launch in front
            float pm[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) pm[k] = th[k];
            compose3(S.ref, pm, th);
        }
    } else if (SRC == XS_SYM && S.kind == 0) {           // theta * [[.1,0,.2],[.1,0,.2]] * 0 + I (ST:503-505): NaN / inf survive
        const float c[6] = {0.1f, 0.0f, 0.2f, 0.1f, 0.0f, 0.2f}, I[6] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f};
        const float *tp = S.theta + (long long)n * 6;
#pragma unroll
        for (int k = 0; k < 6; ++k) th[k] = (tp[k] * c[k]) * 0.0f + I[k];
        th[6] = th[7] = 0.f; th[8] = 1.f;
    } else if (SRC == XS_SYM && S.kind == 1) {           // [theta, 1] * P + [[1,0,0],[0,1,0],[0,0,0]] (ST:692-699)
        const float P[9] = {0.01f, 0.005f, 0.01f, 0.01f, 0.005f, 0.01f, 0.01f, 0.01f, 1.0f}, A[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f};
        const float *tp = S.theta + (long long)n * 8;
#pragma unroll
        for (int k = 0; k < 9; ++k) th[k] = (k < 8 ? tp[k] : 1.0f) * P[k] + A[k];
    } else if (SRC == XS_SYM) {                          // SimilarityTransformer (ST:356-360)
        // six [B] vectors concatenated on axis 0 and reshaped to [B,2,3]: sample n's entry k is vector (6n+k)/B at batch index
        // (6n+k)%B -- for B > 1 the matrices interleave across samples ("BatchSize Should be One", ST:355), restated as is
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const int f = 6 * n + k, v = f / S.B, b = f - v * S.B;
            const float *tp = S.theta + (long long)b * 4;
            const float a = tp[0] * (float)(3.14 / 6) + 0.0f, s = tp[1] * 0.1f + 1.0f;
            float e;
            if (v == 0 || v == 4) e = s * cosf(a);
            else if (v == 1) e = s * sinf(a);
            else if (v == 3) e = (-s) * sinf(a);
            else if (v == 2) e = tp[2] * 0.2f + 0.0f;
            else e = tp[3] * 0.2f + 0.0f;
            th[k] = e;
        }
        th[6] = th[7] = 0.f; th[8] = 1.f;
    }
}

// st_matrix for a whole workgroup: SimilarityTransformer's six entries (cos / sin, the interleave's divisions) are computed by
// six threads into LDS instead of by every thread; the others as st_matrix.  Every thread of the workgroup calls it.
template <int SRC>
__device__ __forceinline__ void st_matrix_wg(const StSrc &S, int n, float *th, float *sm)
{
    if (SRC == XS_SYM && S.kind == 2) {
        if (threadIdx.x == 0) {
            float m[9];
            st_matrix<SRC>(S, n, m);
#pragma unroll
            for (int k = 0; k < 6; ++k) sm[k] = m[k];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 6; ++k) th[k] = sm[k];
        th[6] = th[7] = 0.f; th[8] = 1.f;
    } else if (SRC != XS_COORDS && SRC != XS_TPS) {
        st_matrix<SRC>(S, n, th);
    }
}

// TPS coefficients of sample n into LDS: cf[r*(K+3) + j] = sum_k (src_r[k] + theta[n, r*K+k]) * linv_t[k, j] (ST:108, 145-147), in
// k order, and the control points (lin11 of k % g, k / g) after them for the per-pixel loop.  All threads of the workgroup take
// part; the caller synchronises.
__device__ __forceinline__ void st_tps_coeff(const StSrc &S, int n, float *cf)
{
    const int K = S.g * S.g, K3 = K + 3;
    const float *tp = S.theta + (long long)n * 2 * K;
    for (int k = threadIdx.x; k < K; k += blockDim.x) {          // control points after the coefficients: cp_x[K], cp_y[K]
        cf[2 * K3 + k] = lin11(k % S.g, S.g);
        cf[2 * K3 + K + k] = lin11(k / S.g, S.g);
    }
    for (int e = threadIdx.x; e < 2 * K3; e += blockDim.x) {
        const int r = e / K3, j = e - r * K3;
        float acc = 0.0f;
        for (int k = 0; k < K; ++k) {
            const float src = r == 0 ? lin11(k % S.g, S.g) : lin11(k / S.g, S.g);
            acc = acc + (src + tp[r * K + k]) * S.linv_t[(long long)k * K3 + j];
        }
        cf[e] = acc;
    }
}

// U_func (ST:162-172) of grid point (xt, yt) against the control point (cx, cy): r^2 ln r^2, log 0 = -inf replaced by 0 (ST:166-168).
// The forward's per-pixel loop and the backward's column loop both call it: one fp32 sequence, one set of bits.
__device__ __forceinline__ float st_tps_U(float xt, float yt, float cx, float cy)
{
    const float dx = xt - cx, dy = yt - cy;
    const float r2 = dx * dx + dy * dy;
    return r2 == 0.0f ? 0.0f : r2 * logf(r2);
}

// Affine / ProjectiveTransformer at grid point (xt, yt): T_g = theta . (x_t, y_t, 1), the projective one divided by safe_z (ST:598).
// xh, yh, zs (1 for the affine one) are the values before the division, which the backward's chain rule needs.
__device__ __forceinline__ void st_theta_coords(const float *th, int tdim, float xt, float yt, float &xh, float &yh, float &zs, float &xs, float &ys)
{
    xh = (th[0] * xt + th[1] * yt) + th[2];
    yh = (th[3] * xt + th[4] * yt) + th[5];
    zs = 1.0f; xs = xh; ys = yh;
    if (tdim == 8) {
        zs = (th[6] * xt + th[7] * yt) + 1.0f;
        if (zs == 0.0f) zs = zs + 1e-8f;
        xs = xh / zs;
        ys = yh / zs;
    }
}

// The symmetric-pad transformers at grid point (xt, yt): M . (x_t, y_t, 1) with the pre-mapped matrix, the projective kind divided by
// z as is -- no safe_z (ST:710-711).  xh, yh, zs (1 unless projective) are the values before the division, for the backward's chain rule.
__device__ __forceinline__ void st_sym_coords(const float *th, bool proj, float xt, float yt, float &xh, float &yh, float &zs, float &xs, float &ys)
{
    xh = (th[0] * xt + th[1] * yt) + th[2];
    yh = (th[3] * xt + th[4] * yt) + th[5];
    zs = 1.0f; xs = xh; ys = yh;
    if (proj) {
        zs = (th[6] * xt + th[7] * yt) + th[8];
        xs = xh / zs;
        ys = yh / zs;
    }
}

// normalised source coordinates of grid point (gx, gy) of sample n
template <int SRC>
__device__ __forceinline__ void st_coords(const StSrc &S, const float *th, const float *cf, int n, int gx, int gy, float &xs, float &ys)
{
    if (SRC == XS_COORDS) {
        const long long i = ((long long)n * S.gh + gy) * S.gw + gx;
        xs = S.x[i]; ys = S.y[i];
        return;
    }
    const float xt = st_grid_t(gx, S.sx), yt = st_grid_t(gy, S.sy);
    if (SRC == XS_TPS) {
        const int K = S.g * S.g, K3 = K + 3;
        float ax = (cf[0] * xt + cf[1] * yt) + cf[2];
        float ay = (cf[K3] * xt + cf[K3 + 1] * yt) + cf[K3 + 2];
        const float *cpx = cf + 2 * K3, *cpy = cpx + K;
        for (int k = 0; k < K; ++k) {
            const float U = st_tps_U(xt, yt, cpx[k], cpy[k]);
            ax = ax + cf[3 + k] * U;
            ay = ay + cf[K3 + 3 + k] * U;
        }
        xs = ax; ys = ay;
        return;
    }
    if (SRC == XS_THETA) {
        float xh, yh, zs;
        st_theta_coords(th, S.tdim, xt, yt, xh, yh, zs, xs, ys);
        return;
    }
    float xh, yh, zs;
    st_sym_coords(th, S.kind == 1, xt, yt, xh, yh, zs, xs, ys);
}

// bicubic_interp's taps and weights along one axis (ST:988-1050): clip to [-1,1] first (NaN -> -1), scale, x0 = floor, taps in
// the reference's order [x0, max(x0-1,0), min(x0+1,n-1), min(x0+2,n-1)] (edges replicate: no zero border), alpha = -0.75 weights
// w_i = ((c_i0 + c_i1 t) + c_i2 t^2) + c_i3 t^3.  DERIV (the backward): also the weights' derivatives in t from the same table,
// w'_i = (c_i1 + 2 c_i2 t) + 3 c_i3 t^2 (t = v - floor(v) has derivative 1 in v), and whether the clip passes a gradient:
// -1 <= v <= 1 inclusive, not for NaN -- st_axis_chain's convention for the bilinear clip.
template <bool DERIV = false>
__device__ __forceinline__ void cubic_axis(float v, int n, int *ix, float *w, float *dw = nullptr, bool *pass = nullptr)
{
    const float nf = (float)n;
    if (DERIV) *pass = v >= -1.0f && v <= 1.0f;
    v = fminf(fmaxf(v, -1.0f), 1.0f);
    v = (v + 1.0f) / 2.0f * (nf - 1.0f);
    const float v0f = floorf(v);
    const int v0 = (int)v0f;
    ix[0] = v0; ix[1] = max(v0 - 1, 0); ix[2] = min(v0 + 1, n - 1); ix[3] = min(v0 + 2, n - 1);
    const float t = v - v0f, t2 = t * t, t3 = t2 * t;
    w[0] = ((1.0f + 0.0f * t) + -2.25f * t2) + 1.25f * t3;
    w[1] = ((0.0f + -0.75f * t) + 1.5f * t2) + -0.75f * t3;
    w[2] = ((0.0f + 0.75f * t) + 1.5f * t2) + -1.25f * t3;
    w[3] = ((0.0f + 0.0f * t) + -0.75f * t2) + 0.75f * t3;
    if (DERIV) {
        dw[0] = (0.0f + (2.0f * -2.25f) * t) + (3.0f * 1.25f) * t2;
        dw[1] = (-0.75f + (2.0f * 1.5f) * t) + (3.0f * -0.75f) * t2;
        dw[2] = (0.75f + (2.0f * 1.5f) * t) + (3.0f * -1.25f) * t2;
        dw[3] = (0.0f + (2.0f * -0.75f) * t) + (3.0f * 0.75f) * t2;
    }
}

struct Cubic { int x[4], y[4]; float wx[4], wy[4]; };

// a sampled-extent index to an image index, and the extent the sampler sees: the symmetric pad for XS_SYM, the image otherwise
template <int SRC>
__device__ __forceinline__ int st_src(int p, int n) { return SRC == XS_SYM ? refl(p - 100, n) : p; }
template <int SRC>
__device__ __forceinline__ int st_extent(int n) { return SRC == XS_SYM ? n + 200 : n; }

// final pixel (fx, fy) -> grid point and whether the crop keeps it (only XS_SYM crops or pads)
template <int SRC>
__device__ __forceinline__ bool st_grid_pos(const StSrc &S, int fx, int fy, int &gx, int &gy)
{
    if (SRC != XS_SYM) { gx = fx; gy = fy; return true; }
    const int uy = fy - S.pady, ux = fx - S.padx;
    gy = min(max(uy + S.cropy, 0), S.gh - 1);
    gx = min(max(ux + S.cropx, 0), S.gw - 1);
    return uy >= 0 && uy < S.leny && ux >= 0 && ux < S.lenx;
}

// the bilinear taps of a grid point: from its normalised source coordinates, or (XS_HOMOG) from the homography itself
template <int SRC>
__device__ __forceinline__ Taps st_point_taps(const StSrc &S, const float *th, int gx, int gy, float xs, float ys, int H, int W)
{
    if (SRC == XS_HOMOG) return homog_taps(th, gx, gy, S.dsx, S.dsy, H, W);
    return st_taps(xs, ys, st_extent<SRC>(H), st_extent<SRC>(W));
}

// any channel count, one thread per pixel: workgroups [n * bps, (n + 1) * bps) belong to sample n, so the TPS coefficients are
// computed once per workgroup.  amdgpu_waves_per_eu(4) is there for ONE instantiation, <XS_COORDS, XI_BICUBIC>: the other bicubic
// ones (16 taps in flight) reach four waves per SIMD on their own (124-126 VGPRs), this one the register allocator otherwise lets
// drift to 152; the bilinear instantiations (22-35 VGPRs, eight waves) are not affected.
template <int SRC, int INTERP>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void st_pixel_kernel(const float *__restrict__ img, int H, int W, int C, StSrc S,
                                                       float *__restrict__ out, int FH, int FW, unsigned bps)
{
    __shared__ float cf[SRC == XS_TPS ? 2 * (ST_TPS_KMAX + 3) + 2 * ST_TPS_KMAX : 8];
    const int n = (int)(blockIdx.x / bps);
    if (SRC == XS_TPS) {
        st_tps_coeff(S, n, cf);
        __syncthreads();
    }
    float th[9];
    st_matrix_wg<SRC>(S, n, th, cf);
    const long long p = (long long)(blockIdx.x - (unsigned)n * bps) * 256 + threadIdx.x;
    if (p >= (long long)FH * FW) return;
    const int fy = (int)(p / FW), fx = (int)(p - (long long)fy * FW);
    int gx, gy;
    const bool live = st_grid_pos<SRC>(S, fx, fy, gx, gy);
    float xs = 0.f, ys = 0.f;
    if (SRC != XS_HOMOG) st_coords<SRC>(S, th, cf, n, gx, gy, xs, ys);
    const float *__restrict__ b = img + (long long)n * H * W * C;
    float *__restrict__ o = out + ((long long)n * FH * FW + p) * C;
    if (!live) {                                         // the crop-or-pad padding
        for (int c = 0; c < C; ++c) o[c] = 0.0f;
    } else if (INTERP == XI_BILINEAR) {
        const Taps t = st_point_taps<SRC>(S, th, gx, gy, xs, ys, H, W);
        const long long i00 = ((long long)st_src<SRC>(t.ya, H) * W + st_src<SRC>(t.xa, W)) * C;
        const long long i01 = ((long long)st_src<SRC>(t.ya, H) * W + st_src<SRC>(t.xb, W)) * C;
        const long long i10 = ((long long)st_src<SRC>(t.yb, H) * W + st_src<SRC>(t.xa, W)) * C;
        const long long i11 = ((long long)st_src<SRC>(t.yb, H) * W + st_src<SRC>(t.xb, W)) * C;
        const bool v00 = t.vxa && t.vya, v01 = t.vxb && t.vya, v10 = t.vxa && t.vyb, v11 = t.vxb && t.vyb;
        for (int c = 0; c < C; ++c)
            o[c] = st_blend<SRC == XS_HOMOG>(t, v00 ? b[i00 + c] : 0.f, v01 ? b[i01 + c] : 0.f, v10 ? b[i10 + c] : 0.f, v11 ? b[i11 + c] : 0.f);
    } else {
        Cubic q;
        cubic_axis(xs, st_extent<SRC>(W), q.x, q.wx);
        cubic_axis(ys, st_extent<SRC>(H), q.y, q.wy);
        long long row[4], col[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) { row[i] = (long long)st_src<SRC>(q.y[i], H) * W; col[i] = st_src<SRC>(q.x[i], W); }
        for (int c = 0; c < C; ++c) {
            float r[4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
                r[i] = ((q.wx[0] * b[(row[i] + col[0]) * C + c] + q.wx[1] * b[(row[i] + col[1]) * C + c]) + q.wx[2] * b[(row[i] + col[2]) * C + c])
                       + q.wx[3] * b[(row[i] + col[3]) * C + c];
            o[c] = ((q.wy[0] * r[0] + q.wy[1] * r[1]) + q.wy[2] * r[2]) + q.wy[3] * r[3];
        }
    }
}

// ---------------------------------------------------------------------------------
// 3-channel frames (24 B/px algorithmic: 12 gathered + 12 written, + 8 with explicit coordinates).
// Shaped like tf_warp's tile kernel (flow_ops.hip, warp3_tile_kernel; profiles/README.md "r02 warp study"): a workgroup owns a
// 16 x 32 tile of ONE sample's output pixels and a wave instruction works on a 4 x 16 patch, so the lines a gather touches are a
// compact 2-D footprint under any rotation; one 3-dword load per tap; results leave through LDS as 16-byte stores of whole
// 384-byte tile rows (ow % 4 == 0; 12-byte stores otherwise); XCD-contiguous tile order.
// Measured and rejected twice (profiles/README.md "r03 sampler study"): staging the source window in LDS -- bounding box of the taps
// by DPP reductions, aligned 16-byte fill, corners from LDS -- cuts the L1 lookups 3x (0.50 instead of 1.56 per pixel) and is
// SLOWER both per workgroup tile (commit 2076632: four barriers, three dependent phases; 0.34-0.39 of 8 TB/s against 0.53-0.65)
// and per wave patch with no barrier at all (0.41-0.49): what bounds these kernels is requests in flight, not tag lookups.  So the
// bilinear path of the theta, coordinate and homography sources issues the gathers of both of a thread's pixels before it blends
// either (arrays over PPT).  Bicubic gathers 16 taps per pixel, row by row in tap order, one pixel at a time: both pixels' 32 taps
// in flight cost registers and occupancy.
// ---------------------------------------------------------------------------------
using StTile = Tile3<>;

template <int SRC, bool STAGE, int INTERP>
__global__ __launch_bounds__(256) void st3_tile_kernel(const float *__restrict__ img, int H, int W, StSrc S,
                                                       float *__restrict__ out, int FH, int FW, int tiles_x, int tiles_y)
{
    constexpr int PPT = StTile::PPT;
    __shared__ __attribute__((aligned(16))) float lds[STAGE ? StTile::TH * StTile::TW * 3 : 4];
    __shared__ float cf[SRC == XS_TPS ? 2 * (ST_TPS_KMAX + 3) + 2 * ST_TPS_KMAX : 8];
    const StTile tile(tiles_x, tiles_y);
    const int n = tile.n;
    if (SRC == XS_TPS) {
        st_tps_coeff(S, n, cf);
        __syncthreads();
    }
    float th[9];
    st_matrix_wg<SRC>(S, n, th, cf);
    const rgb3 *b = reinterpret_cast<const rgb3 *>(img) + (long long)n * H * W;     // 3 B H W < 2^31 (host)
    int yy[PPT], xx[PPT];
    bool ok[PPT], live[PPT];
    float xs[PPT], ys[PPT];
    Taps t[PPT];
    // pass j's pixel: its source coordinates and, for the bilinear sampler, its taps
    auto point = [&](int j) {
        ok[j] = tile.y(j) < FH && tile.x(j) < FW;
        yy[j] = min(tile.y(j), FH - 1); xx[j] = min(tile.x(j), FW - 1);          // a pixel beyond the output repeats an edge pixel of this tile (not stored)
        int gx, gy;
        live[j] = st_grid_pos<SRC>(S, xx[j], yy[j], gx, gy);
        if (SRC != XS_HOMOG) st_coords<SRC>(S, th, cf, n, gx, gy, xs[j], ys[j]);
        if (INTERP == XI_BILINEAR) t[j] = st_point_taps<SRC>(S, th, gx, gy, xs[j], ys[j], H, W);
    };
    auto put = [&](int j, rgb3 r) {
        if (!live[j]) r.r = r.g = r.b = 0.0f;
        if (STAGE) *reinterpret_cast<rgb3 *>(lds + tile.staged(j) * 3) = r;
        else if (ok[j]) reinterpret_cast<rgb3 *>(out)[((long long)n * FH + yy[j]) * FW + xx[j]] = r;
    };
    if (INTERP == XI_BILINEAR) {
        rgb3 I00[PPT], I01[PPT], I10[PPT], I11[PPT];
        auto gather = [&](int j) {
            const int ya = st_src<SRC>(t[j].ya, H) * W, yb = st_src<SRC>(t[j].yb, H) * W, xa = st_src<SRC>(t[j].xa, W), xb = st_src<SRC>(t[j].xb, W);
            I00[j] = b[ya + xa]; I01[j] = b[ya + xb]; I10[j] = b[yb + xa]; I11[j] = b[yb + xb];
        };
        auto blend = [&](int j) {
            const bool v00 = t[j].vxa && t[j].vya, v01 = t[j].vxb && t[j].vya, v10 = t[j].vxa && t[j].vyb, v11 = t[j].vxb && t[j].vyb;
            rgb3 r;
            r.r = st_blend<SRC == XS_HOMOG>(t[j], v00 ? I00[j].r : 0.f, v01 ? I01[j].r : 0.f, v10 ? I10[j].r : 0.f, v11 ? I11[j].r : 0.f);
            r.g = st_blend<SRC == XS_HOMOG>(t[j], v00 ? I00[j].g : 0.f, v01 ? I01[j].g : 0.f, v10 ? I10[j].g : 0.f, v11 ? I11[j].g : 0.f);
            r.b = st_blend<SRC == XS_HOMOG>(t[j], v00 ? I00[j].b : 0.f, v01 ? I01[j].b : 0.f, v10 ? I10[j].b : 0.f, v11 ? I11[j].b : 0.f);
            put(j, r);
        };
        // The gathers of both pixels are issued before either is blended (requests in flight, above).  The symmetric-pad and
        // thin-plate-spline sources, heavier per pixel, keep the one-pixel-at-a-time order they were written and measured in
        // (DESIGN.md section 11); both in flight was 2-3 % slower for the symmetric-pad ones when tried.
        if (SRC == XS_SYM || SRC == XS_TPS) {
#pragma unroll
            for (int j = 0; j < PPT; ++j) { point(j); gather(j); blend(j); }
        } else {
#pragma unroll
            for (int j = 0; j < PPT; ++j) point(j);
#pragma unroll
            for (int j = 0; j < PPT; ++j) gather(j);
#pragma unroll
            for (int j = 0; j < PPT; ++j) blend(j);
        }
    } else {                                         // one pixel at a time
#pragma unroll
        for (int j = 0; j < PPT; ++j) {
            point(j);
            Cubic c;
            cubic_axis(xs[j], st_extent<SRC>(W), c.x, c.wx);
            cubic_axis(ys[j], st_extent<SRC>(H), c.y, c.wy);
            int col[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) col[i] = st_src<SRC>(c.x[i], W);
            rgb3 rw[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int ro = st_src<SRC>(c.y[i], H) * W;
                const rgb3 I0 = b[ro + col[0]], I1 = b[ro + col[1]], I2 = b[ro + col[2]], I3 = b[ro + col[3]];
                rw[i].r = ((c.wx[0] * I0.r + c.wx[1] * I1.r) + c.wx[2] * I2.r) + c.wx[3] * I3.r;
                rw[i].g = ((c.wx[0] * I0.g + c.wx[1] * I1.g) + c.wx[2] * I2.g) + c.wx[3] * I3.g;
                rw[i].b = ((c.wx[0] * I0.b + c.wx[1] * I1.b) + c.wx[2] * I2.b) + c.wx[3] * I3.b;
            }
            rgb3 r;
            r.r = ((c.wy[0] * rw[0].r + c.wy[1] * rw[1].r) + c.wy[2] * rw[2].r) + c.wy[3] * rw[3].r;
            r.g = ((c.wy[0] * rw[0].g + c.wy[1] * rw[1].g) + c.wy[2] * rw[2].g) + c.wy[3] * rw[3].g;
            r.b = ((c.wy[0] * rw[0].b + c.wy[1] * rw[1].b) + c.wy[2] * rw[2].b) + c.wy[3] * rw[3].b;
            put(j, r);
        }
    }
    if (STAGE) tile.template store_rows<3>(lds, out, FH, FW);          // FW % 4 == 0 (host): a tile row is TW*12 bytes from a 16-byte aligned address
}

// a source's fp32 linspace steps 2/(n-1), divided once on the host (the same IEEE quotient lin11 computes)
static void st_steps(StSrc &S)
{
    S.sx = S.gw > 1 ? 2.0f / (float)(S.gw - 1) : 0.0f; S.sy = S.gh > 1 ? 2.0f / (float)(S.gh - 1) : 0.0f;
}

// Picks the kernel of a launch: the tile kernel for 3-channel frames of a shape that is its own, the pixel kernel otherwise.
// `slot` / `px_bytes`: the launch_timed slot and algorithmic bytes per output pixel of the tile launch (slot < 0: not timed).
template <int SRC, int INTERP>
static hipError_t launch_st(int slot, double px_bytes, const float *img, int B, int H, int W, int C, StSrc S, float *out, int FH, int FW,
                            hipStream_t stream)
{
    S.B = B;
    st_steps(S);
    S.dsx = S.gw > 1 ? 2.0 / (double)(S.gw - 1) : 0.0; S.dsy = S.gh > 1 ? 2.0 / (double)(S.gh - 1) : 0.0;
    int tx, ty;
    dim3 grid;
    if (C == 3 && StTile::plan(B, FH, FW, 3 * std::max((long long)B * H * W, (long long)B * FH * FW), tx, ty, grid)) {
        const double bytes = px_bytes * B * FH * FW;       // every output pixel reads ~one source pixel, writes one (+ x, y)
        if (StTile::staged_ok(out, FW, 3))
            return launch_timed(slot, bytes, st3_tile_kernel<SRC, true, INTERP>, grid, dim3(256), stream, img, H, W, S, out, FH, FW, tx, ty);
        return launch_timed(slot, bytes, st3_tile_kernel<SRC, false, INTERP>, grid, dim3(256), stream, img, H, W, S, out, FH, FW, tx, ty);
    }
    const long long bps = ((long long)FH * FW + 255) / 256;
    if (bps * B >= (1ll << 31)) return hipErrorInvalidValue;
    st_pixel_kernel<SRC, INTERP><<<dim3((unsigned)(bps * B)), dim3(256), 0, stream>>>(img, H, W, C, S, out, FH, FW, (unsigned)bps);
    return hipGetLastError();
}

// a source whose sampling grid is the output: no crop, no pad
static StSrc st_plain(int oh, int ow)
{
    StSrc S{};
    S.gh = oh; S.gw = ow;
    return S;
}

hipError_t launch_st_interp(const float *img, int B, int H, int W, int C, const float *x, const float *y, int oh, int ow, float *out,
                            hipStream_t stream)
{
    StSrc S = st_plain(oh, ow);
    S.x = x; S.y = y;
    return launch_st<XS_COORDS, XI_BILINEAR>(HBM_SLOT_ST, 32.0, img, B, H, W, C, S, out, oh, ow, stream);
}

hipError_t launch_st_transform(const float *img, int B, int H, int W, int C, const float *theta, int tdim, float *out, int oh,
                               int ow, hipStream_t stream)
{
    StSrc S = st_plain(oh, ow);
    S.theta = theta; S.tdim = tdim;
    return launch_st<XS_THETA, XI_BILINEAR>(HBM_SLOT_ST, 24.0, img, B, H, W, C, S, out, oh, ow, stream);
}

hipError_t launch_homography_warp(const float *img, int B, int Hi, int Wi, int C, const float *M, float *out, int oh, int ow,
                                  hipStream_t stream, const float *ref)
{
    StSrc S = st_plain(oh, ow);
    S.theta = M; S.tdim = 9; S.ref = ref;
    return launch_st<XS_HOMOG, XI_BILINEAR>(HBM_SLOT_HOMOG, 24.0, img, B, Hi, Wi, C, S, out, oh, ow, stream);
}

hipError_t launch_st_meshgrid(float *out, int oh, int ow, hipStream_t stream)
{
    st_meshgrid_kernel<<<dim3((unsigned)((oh * ow + 255) / 256)), dim3(256), 0, stream>>>(out, oh, ow);
    return hipGetLastError();
}

// warp.vec2mtrx (warp.py:25-43): sl(3) / affine generator -> matrix exponential by Taylor series,
// pMtrx = sum_{i=0}^{warpApprox-1} A^i / i!   (fp32, one thread per batch element)
__global__ void vec2mtrx_kernel(const float *__restrict__ p, int B, int dim, int approx, float *__restrict__ out)
{
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= B) return;
    const float *q = p + (long long)n * dim;
    float A[9];
    if (dim == 8) {
        A[0] = q[2]; A[1] = q[1]; A[2] = q[0];
        A[3] = q[5]; A[4] = -q[2] - q[6]; A[5] = q[4];
        A[6] = q[3]; A[7] = q[7]; A[8] = q[6];
    } else {
        A[0] = q[0]; A[1] = q[1]; A[2] = q[2];
        A[3] = q[3]; A[4] = q[4]; A[5] = q[5];
        A[6] = 0.f; A[7] = 0.f; A[8] = 0.f;
    }
    float P[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, Nm[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    float denom = 1.0f;
    for (int i = 1; i < approx; ++i) {
        float T[9];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) T[r * 3 + c] = (Nm[r * 3] * A[c] + Nm[r * 3 + 1] * A[3 + c]) + Nm[r * 3 + 2] * A[6 + c];
        denom *= (float)i;
        for (int k = 0; k < 9; ++k) { Nm[k] = T[k]; P[k] += T[k] / denom; }
    }
    for (int k = 0; k < 9; ++k) out[(long long)n * 9 + k] = P[k];
}

hipError_t launch_vec2mtrx(const float *p, int B, int dim, int approx, float *out, hipStream_t stream)
{
    vec2mtrx_kernel<<<dim3((unsigned)((B + 63) / 64)), dim3(64), 0, stream>>>(p, B, dim, approx, out);
    return hipGetLastError();
}

hipError_t launch_st_bicubic_interp(const float *img, int B, int H, int W, int C, const float *x, const float *y, int oh, int ow,
                                    float *out, hipStream_t stream)
{
    StSrc S = st_plain(oh, ow);
    S.x = x; S.y = y;
    return launch_st<XS_COORDS, XI_BICUBIC>(-1, 0.0, img, B, H, W, C, S, out, oh, ow, stream);
}

hipError_t launch_st_transform_interp(const float *img, int B, int H, int W, int C, const float *theta, int tdim, int interp,
                                      float *out, int oh, int ow, hipStream_t stream)
{
    if (interp == XI_BILINEAR) return launch_st_transform(img, B, H, W, C, theta, tdim, out, oh, ow, stream);
    StSrc S = st_plain(oh, ow);
    S.theta = theta; S.tdim = tdim;
    return launch_st<XS_THETA, XI_BICUBIC>(-1, 0.0, img, B, H, W, C, S, out, oh, ow, stream);
}

// the symmetric-pad source of out_size (oh, ow): the (oh+200) x (ow+200) sampling grid and the crop-or-pad to th x tw, the final extent
static StSrc st_sym_src(const float *theta, int kind, int oh, int ow, int &th, int &tw)
{
    StSrc S{};
    S.theta = theta; S.kind = kind;
    S.tdim = kind == 1 ? 8 : 6;              // the backward's d M entries per sample (st_theta_accum)
    S.gh = oh + 200; S.gw = ow + 200;
    // resize_image_with_crop_or_pad(out, ow, oh) (ST:343, 488, 682): target height ow, width oh -- swapped
    th = ow; tw = oh;
    S.cropy = max((S.gh - th) / 2, 0); S.pady = max((th - S.gh) / 2, 0); S.leny = min(S.gh, th);
    S.cropx = max((S.gw - tw) / 2, 0); S.padx = max((tw - S.gw) / 2, 0); S.lenx = min(S.gw, tw);
    return S;
}

hipError_t launch_st_symmetry_transform(const float *img, int B, int H, int W, int C, const float *theta, int kind, int interp,
                                        float *out, int oh, int ow, hipStream_t stream)
{
    int th, tw;
    const StSrc S = st_sym_src(theta, kind, oh, ow, th, tw);
    if (interp == XI_BILINEAR) return launch_st<XS_SYM, XI_BILINEAR>(-1, 0.0, img, B, H, W, C, S, out, th, tw, stream);
    return launch_st<XS_SYM, XI_BICUBIC>(-1, 0.0, img, B, H, W, C, S, out, th, tw, stream);
}

hipError_t launch_st_elastic_transform(const float *img, int B, int H, int W, int C, const float *theta, int g, const float *linv_t,
                                       int interp, float *out, int oh, int ow, hipStream_t stream)
{
    StSrc S = st_plain(oh, ow);
    S.theta = theta; S.g = g; S.linv_t = linv_t;
    if (interp == XI_BILINEAR) return launch_st<XS_TPS, XI_BILINEAR>(-1, 0.0, img, B, H, W, C, S, out, oh, ow, stream);
    return launch_st<XS_TPS, XI_BICUBIC>(-1, 0.0, img, B, H, W, C, S, out, oh, ow, stream);
}

// ElasticTransformer's normalised source coordinates themselves (the x_s_flat, y_s_flat of ST:140-158), [B*oh*ow] each: st_tps_coeff
// and st_coords<XS_TPS>, called as the sampling kernels call them, so these are the values the forward samples at bit for bit.
// st_pixel_kernel's layout: workgroups [n * bps, (n + 1) * bps) belong to sample n.
__global__ __launch_bounds__(256) void st_tps_coords_kernel(StSrc S, float *__restrict__ x_out, float *__restrict__ y_out, int FH, int FW, unsigned bps)
{
    __shared__ float cf[2 * (ST_TPS_KMAX + 3) + 2 * ST_TPS_KMAX];
    const int n = (int)(blockIdx.x / bps);
    st_tps_coeff(S, n, cf);
    __syncthreads();
    const long long p = (long long)(blockIdx.x - (unsigned)n * bps) * 256 + threadIdx.x;
    if (p >= (long long)FH * FW) return;
    const int fy = (int)(p / FW), fx = (int)(p - (long long)fy * FW);
    float xs, ys;
    st_coords<XS_TPS>(S, nullptr, cf, n, fx, fy, xs, ys);
    x_out[(long long)n * FH * FW + p] = xs;
    y_out[(long long)n * FH * FW + p] = ys;
}

static StSrc st_elastic_src(int B, const float *theta, int g, const float *linv_t, int oh, int ow)
{
    StSrc S = st_plain(oh, ow);
    S.theta = theta; S.g = g; S.linv_t = linv_t; S.B = B;
    st_steps(S);
    return S;
}

hipError_t launch_st_elastic_coords(const float *theta, int B, int g, const float *linv_t, int oh, int ow, float *x_out, float *y_out,
                                    hipStream_t stream)
{
    const long long bps = ((long long)oh * ow + 255) / 256;
    if (bps * B >= (1ll << 31)) return hipErrorInvalidValue;
    st_tps_coords_kernel<<<dim3((unsigned)(bps * B)), dim3(256), 0, stream>>>(st_elastic_src(B, theta, g, linv_t, oh, ow), x_out, y_out, oh, ow,
                                                                              (unsigned)bps);
    return hipGetLastError();
}

// The symmetric-pad transformers' pre-mapped matrices themselves, [B,9] (SimilarityTransformer's interleave included), and their
// normalised source coordinates per FINAL pixel, [B*FH*FW] each (0 where the crop-or-pad pads): st_matrix / st_matrix_wg, st_grid_pos
// and st_coords<XS_SYM>, called as the sampling kernels call them, so these are the values the forward uses bit for bit.
__global__ __launch_bounds__(64) void st_sym_matrix_kernel(StSrc S, float *__restrict__ out)
{
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= S.B) return;
    float th[9];
    st_matrix<XS_SYM>(S, n, th);
#pragma unroll
    for (int k = 0; k < 9; ++k) out[(long long)n * 9 + k] = th[k];
}

__global__ __launch_bounds__(256) void st_sym_coords_kernel(StSrc S, float *__restrict__ x_out, float *__restrict__ y_out, int FH, int FW, unsigned bps)
{
    __shared__ float sm[8];
    const int n = (int)(blockIdx.x / bps);
    float th[9];
    st_matrix_wg<XS_SYM>(S, n, th, sm);
    const long long p = (long long)(blockIdx.x - (unsigned)n * bps) * 256 + threadIdx.x;
    if (p >= (long long)FH * FW) return;
    const int fy = (int)(p / FW), fx = (int)(p - (long long)fy * FW);
    int gx, gy;
    float xs = 0.f, ys = 0.f;
    if (st_grid_pos<XS_SYM>(S, fx, fy, gx, gy)) st_coords<XS_SYM>(S, th, nullptr, n, gx, gy, xs, ys);
    x_out[(long long)n * FH * FW + p] = xs;
    y_out[(long long)n * FH * FW + p] = ys;
}

hipError_t launch_st_symmetry_matrix(const float *theta, int B, int kind, float *out, hipStream_t stream)
{
    int th, tw;
    StSrc S = st_sym_src(theta, kind, 1, 1, th, tw);
    S.B = B;
    st_sym_matrix_kernel<<<dim3((unsigned)((B + 63) / 64)), dim3(64), 0, stream>>>(S, out);
    return hipGetLastError();
}

hipError_t launch_st_symmetry_coords(const float *theta, int B, int kind, int oh, int ow, float *x_out, float *y_out, hipStream_t stream)
{
    int th, tw;
    StSrc S = st_sym_src(theta, kind, oh, ow, th, tw);
    S.B = B;
    st_steps(S);
    const long long bps = ((long long)th * tw + 255) / 256;
    if (bps * B >= (1ll << 31)) return hipErrorInvalidValue;
    st_sym_coords_kernel<<<dim3((unsigned)(bps * B)), dim3(256), 0, stream>>>(S, x_out, y_out, th, tw, (unsigned)bps);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------
// Backward of the BILINEAR sampler for the theta (affine / projective) and explicit-coordinate sources: what TensorFlow's autodiff
// gives for ST:902-964 and ST:438-452 / 578-608.  The coordinates, taps and weights are the forward's (st_theta_coords, st_axis,
// st_taps), so the backward's tap decisions are the forward's.
//   d img    the adjoint of the gather, w_k * dout added to the four taps (none to a tap on the zero border), by float atomics:
//            the result DEPENDS ON ATOMIC ARRIVAL ORDER IN ITS LAST BITS.  Four global atomics per pixel-channel, for any channel
//            count and any theta.  A form that sums a tile's contributions in an LDS window first is NOT built.
//   d x, d y per pixel: floor and the int casts have zero derivative, so per channel d out / d x = (I01 - I00) (y1f - y) +
//            (I11 - I10) (y - y0f) in padded-pixel units (st_slope), summed over the channels times dout, passed by the clip where
//            -1 <= x <= W inclusive (0 for NaN), times (W - 1) / 2.  Stored for explicit coordinates.
//   d theta  the per-pixel products (gx x_t, gx y_t, gx, gy x_t, gy y_t, gy; the projective chain through x_h / safe_z in double
//            from the forward's fp32 x_h, y_h, safe_z) summed over the pixels in double: per thread, per wave (shuffles), per
//            workgroup (LDS) into part[workgroup][8], then st_theta_final_kernel in a fixed order -- bit-reproducible, no atomics.
// ---------------------------------------------------------------------------------
// one channel's share of d out / d (x, y), in padded-pixel units, times its dout
__device__ __forceinline__ void st_slope(const Axis &X, const Axis &Y, float I00, float I01, float I10, float I11, float g, float &gx, float &gy)
{
    gx = gx + ((I01 - I00) * Y.hi + (I11 - I10) * Y.lo) * g;
    gy = gy + ((I10 - I00) * X.hi + (I11 - I01) * X.lo) * g;
}

// a pixel's share of d theta, added to acc[8] in double: d x_h = gx / z, d y_h = gy / z, d z = -(gx x_h + gy y_h) / z^2
__device__ __forceinline__ void st_theta_accum(double *acc, int tdim, float gxn, float gyn, float xt, float yt, float xh, float yh, float zs)
{
    if (gxn == 0.0f && gyn == 0.0f) return;
    double gx = (double)gxn, gy = (double)gyn;
    if (tdim == 8) {
        const double iz = 1.0 / (double)zs;
        const double gz = -(gx * (double)xh + gy * (double)yh) * iz * iz;
        gx *= iz; gy *= iz;
        acc[6] += gz * (double)xt; acc[7] += gz * (double)yt;
    }
    acc[0] += gx * (double)xt; acc[1] += gx * (double)yt; acc[2] += gx;
    acc[3] += gy * (double)xt; acc[4] += gy * (double)yt; acc[5] += gy;
}

struct StBwd {
    const float *dout;             // [B, FH, FW, C]
    float *d_img;                  // [B, H, W, C], added to (null: not wanted)
    float *d_x, *d_y;              // XS_COORDS [B*FH*FW] (each nullable)
    double *part;                  // XS_THETA [workgroups][8] (null: d theta not wanted)
};

// The bilinear backward of ONE output pixel sampled at (xs, ys), stated once for every source of coordinates.  b, di: the sample's
// image and its gradient; g: the pixel's dout.  DIMG: w_k * dout added to the four taps (none to a tap on the zero border).  DCOORD:
// gxn, gyn = d out / d (xs, ys) summed over the channels times dout, through the clip and the pixel scaling (0 otherwise).
// XS_SYM: the axes are the padded extent's (st_extent) and a padded tap p is image pixel refl(p - 100) (st_src), for the values read
// and for the adjoint alike: several padded taps fold onto one image pixel and all of them add.  Any channel count:
template <bool DIMG, bool DCOORD, int SRC = XS_THETA>
__device__ __forceinline__ void st_bwd_point(const float *__restrict__ b, float *di, const float *__restrict__ g, int H, int W, int C, float xs,
                                             float ys, float &gxn, float &gyn)
{
    const Axis X = st_axis(xs, st_extent<SRC>(W)), Y = st_axis(ys, st_extent<SRC>(H));
    const Taps t = st_taps(X, Y);
    const int ya = st_src<SRC>(t.ya, H), yb = st_src<SRC>(t.yb, H), xa = st_src<SRC>(t.xa, W), xb = st_src<SRC>(t.xb, W);
    const long long i00 = ((long long)ya * W + xa) * C, i01 = ((long long)ya * W + xb) * C;
    const long long i10 = ((long long)yb * W + xa) * C, i11 = ((long long)yb * W + xb) * C;
    const bool v00 = t.vxa && t.vya, v01 = t.vxb && t.vya, v10 = t.vxa && t.vyb, v11 = t.vxb && t.vyb;
    float gx = 0.f, gy = 0.f;
    for (int c = 0; c < C; ++c) {
        const float gc = g[c];
        if (DCOORD) st_slope(X, Y, v00 ? b[i00 + c] : 0.f, v01 ? b[i01 + c] : 0.f, v10 ? b[i10 + c] : 0.f, v11 ? b[i11 + c] : 0.f, gc, gx, gy);
        if (DIMG) {
            if (v00) atomicAdd(di + i00 + c, t.w0 * gc);
            if (v01) atomicAdd(di + i01 + c, t.w1 * gc);
            if (v10) atomicAdd(di + i10 + c, t.w2 * gc);
            if (v11) atomicAdd(di + i11 + c, t.w3 * gc);
        }
    }
    gxn = DCOORD ? st_axis_chain(X, gx, st_extent<SRC>(W)) : 0.0f;
    gyn = DCOORD ? st_axis_chain(Y, gy, st_extent<SRC>(H)) : 0.0f;
}

// 3-channel frames (3 H W < 2^31: host):
template <bool DIMG, bool DCOORD, int SRC = XS_THETA>
__device__ __forceinline__ void st3_bwd_point(const rgb3 *b, float *di, const rgb3 g, int H, int W, float xs, float ys, float &gxn, float &gyn)
{
    const Axis X = st_axis(xs, st_extent<SRC>(W)), Y = st_axis(ys, st_extent<SRC>(H));
    const Taps t = st_taps(X, Y);
    const int ya = st_src<SRC>(t.ya, H), yb = st_src<SRC>(t.yb, H), xa = st_src<SRC>(t.xa, W), xb = st_src<SRC>(t.xb, W);
    const bool v00 = t.vxa && t.vya, v01 = t.vxb && t.vya, v10 = t.vxa && t.vyb, v11 = t.vxb && t.vyb;
    gxn = gyn = 0.0f;
    if (DCOORD) {
        const rgb3 z = {0.f, 0.f, 0.f};
        const rgb3 I00 = v00 ? b[ya * W + xa] : z, I01 = v01 ? b[ya * W + xb] : z;
        const rgb3 I10 = v10 ? b[yb * W + xa] : z, I11 = v11 ? b[yb * W + xb] : z;
        float gx = 0.f, gy = 0.f;
        st_slope(X, Y, I00.r, I01.r, I10.r, I11.r, g.r, gx, gy);
        st_slope(X, Y, I00.g, I01.g, I10.g, I11.g, g.g, gx, gy);
        st_slope(X, Y, I00.b, I01.b, I10.b, I11.b, g.b, gx, gy);
        gxn = st_axis_chain(X, gx, st_extent<SRC>(W)); gyn = st_axis_chain(Y, gy, st_extent<SRC>(H));
    }
    if (DIMG) {
        auto add = [&](int y, int x, bool valid, float w) {
            if (!valid) return;
            float *q = di + ((long long)y * W + x) * 3;
            atomicAdd(q, w * g.r); atomicAdd(q + 1, w * g.g); atomicAdd(q + 2, w * g.b);
        };
        add(ya, xa, v00, t.w0); add(ya, xb, v01, t.w1); add(yb, xa, v10, t.w2); add(yb, xb, v11, t.w3);
    }
}

// ---------------------------------------------------------------------------------
// Backward of the BICUBIC sampler (XI_BICUBIC) for the theta, explicit-coordinate, symmetric-pad and thin-plate-spline sources: what
// TensorFlow's autodiff gives for ST:966-1072, out_c = sum_i sum_j wy_i wx_j I[ys_i, xs_j, c].  Taps and weights are cubic_axis's, the
// forward's own, so every floor, clip and edge decision is shared.  One tap row at a time, so that no more than four taps are held:
//   d img    the gather's adjoint, wx_j * (wy_i * dout_c) added to each of the 16 taps by float atomics (arrival order in the last
//            bits).  The replicate-clamp folds several taps onto one edge pixel and all of them add: there is no zero border.  XS_SYM:
//            the taps are the padded extent's (st_extent) mapped through st_src, as in the forward.
//   d x, d y floor and the int casts have zero derivative, t = v - floor(v) has derivative 1: per channel d out / d x =
//            sum_i wy_i (sum_j w'x_j I_ij), d out / d y = sum_i w'y_i (sum_j wx_j I_ij), each times dout, summed over the channels,
//            times (W - 1) / 2 (H for y).  The clip to [-1,1] passes the gradient where -1 <= x <= 1 inclusive, 0 outside and for NaN
//            (which the forward reads as -1): st_axis_chain's convention.
// gxn, gyn feed each source's d theta chain unchanged (st_theta_accum, the symmetric-pad pre-map, the TPS coefficient sums).
// ---------------------------------------------------------------------------------
__device__ __forceinline__ float cubic_chain(bool pass, float g, int n) { return pass ? g * (((float)n - 1.0f) / 2.0f) : 0.0f; }

// any channel count:
template <bool DIMG, bool DCOORD, int SRC = XS_THETA>
__device__ __forceinline__ void st_cubic_bwd_point(const float *__restrict__ b, float *di, const float *__restrict__ g, int H, int W, int C, float xs,
                                                   float ys, float &gxn, float &gyn)
{
    Cubic q;
    float dwx[4], dwy[4];
    bool px = false, py = false;
    cubic_axis<DCOORD>(xs, st_extent<SRC>(W), q.x, q.wx, dwx, &px);
    cubic_axis<DCOORD>(ys, st_extent<SRC>(H), q.y, q.wy, dwy, &py);
    long long row[4], col[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { row[i] = (long long)st_src<SRC>(q.y[i], H) * W; col[i] = st_src<SRC>(q.x[i], W); }
    float gx = 0.f, gy = 0.f;
    for (int c = 0; c < C; ++c) {
        const float gc = g[c];
        float sx = 0.f, sy = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long long i0 = (row[i] + col[0]) * C + c, i1 = (row[i] + col[1]) * C + c, i2 = (row[i] + col[2]) * C + c, i3 = (row[i] + col[3]) * C + c;
            if (DCOORD) {
                const float I0 = b[i0], I1 = b[i1], I2 = b[i2], I3 = b[i3];
                const float r = ((q.wx[0] * I0 + q.wx[1] * I1) + q.wx[2] * I2) + q.wx[3] * I3;
                const float d = ((dwx[0] * I0 + dwx[1] * I1) + dwx[2] * I2) + dwx[3] * I3;
                sx = sx + q.wy[i] * d;
                sy = sy + dwy[i] * r;
            }
            if (DIMG) {
                const float wg = q.wy[i] * gc;
                atomicAdd(di + i0, q.wx[0] * wg); atomicAdd(di + i1, q.wx[1] * wg);
                atomicAdd(di + i2, q.wx[2] * wg); atomicAdd(di + i3, q.wx[3] * wg);
            }
        }
        gx = gx + sx * gc;
        gy = gy + sy * gc;
    }
    gxn = DCOORD ? cubic_chain(px, gx, st_extent<SRC>(W)) : 0.0f;
    gyn = DCOORD ? cubic_chain(py, gy, st_extent<SRC>(H)) : 0.0f;
}

// 3-channel frames (3 H W < 2^31: host): the same sums in the same order, a tap read as one 3-dword load
template <bool DIMG, bool DCOORD, int SRC = XS_THETA>
__device__ __forceinline__ void st3_cubic_bwd_point(const rgb3 *b, float *di, const rgb3 g, int H, int W, float xs, float ys, float &gxn, float &gyn)
{
    Cubic q;
    float dwx[4], dwy[4];
    bool px = false, py = false;
    cubic_axis<DCOORD>(xs, st_extent<SRC>(W), q.x, q.wx, dwx, &px);
    cubic_axis<DCOORD>(ys, st_extent<SRC>(H), q.y, q.wy, dwy, &py);
    int col[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) col[j] = st_src<SRC>(q.x[j], W);
    rgb3 sx = {0.f, 0.f, 0.f}, sy = {0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int ro = st_src<SRC>(q.y[i], H) * W;
        if (DCOORD) {
            const rgb3 I0 = b[ro + col[0]], I1 = b[ro + col[1]], I2 = b[ro + col[2]], I3 = b[ro + col[3]];
            sx.r = sx.r + q.wy[i] * (((dwx[0] * I0.r + dwx[1] * I1.r) + dwx[2] * I2.r) + dwx[3] * I3.r);
            sx.g = sx.g + q.wy[i] * (((dwx[0] * I0.g + dwx[1] * I1.g) + dwx[2] * I2.g) + dwx[3] * I3.g);
            sx.b = sx.b + q.wy[i] * (((dwx[0] * I0.b + dwx[1] * I1.b) + dwx[2] * I2.b) + dwx[3] * I3.b);
            sy.r = sy.r + dwy[i] * (((q.wx[0] * I0.r + q.wx[1] * I1.r) + q.wx[2] * I2.r) + q.wx[3] * I3.r);
            sy.g = sy.g + dwy[i] * (((q.wx[0] * I0.g + q.wx[1] * I1.g) + q.wx[2] * I2.g) + q.wx[3] * I3.g);
            sy.b = sy.b + dwy[i] * (((q.wx[0] * I0.b + q.wx[1] * I1.b) + q.wx[2] * I2.b) + q.wx[3] * I3.b);
        }
        if (DIMG) {
            const float wr = q.wy[i] * g.r, wg = q.wy[i] * g.g, wb = q.wy[i] * g.b;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float *p = di + ((long long)ro + col[j]) * 3;
                atomicAdd(p, q.wx[j] * wr); atomicAdd(p + 1, q.wx[j] * wg); atomicAdd(p + 2, q.wx[j] * wb);
            }
        }
    }
    gxn = gyn = 0.0f;
    if (DCOORD) {
        const float gx = (sx.r * g.r + sx.g * g.g) + sx.b * g.b, gy = (sy.r * g.r + sy.g * g.g) + sy.b * g.b;
        gxn = cubic_chain(px, gx, st_extent<SRC>(W)); gyn = cubic_chain(py, gy, st_extent<SRC>(H));
    }
}

// a pixel's backward with the sampler of the launch
template <bool DIMG, bool DCOORD, int SRC, int INTERP>
__device__ __forceinline__ void st_point_bwd(const float *__restrict__ b, float *di, const float *__restrict__ g, int H, int W, int C, float xs, float ys,
                                             float &gxn, float &gyn)
{
    if (INTERP == XI_BICUBIC) st_cubic_bwd_point<DIMG, DCOORD, SRC>(b, di, g, H, W, C, xs, ys, gxn, gyn);
    else st_bwd_point<DIMG, DCOORD, SRC>(b, di, g, H, W, C, xs, ys, gxn, gyn);
}
template <bool DIMG, bool DCOORD, int SRC, int INTERP>
__device__ __forceinline__ void st3_point_bwd(const rgb3 *b, float *di, const rgb3 g, int H, int W, float xs, float ys, float &gxn, float &gyn)
{
    if (INTERP == XI_BICUBIC) st3_cubic_bwd_point<DIMG, DCOORD, SRC>(b, di, g, H, W, xs, ys, gxn, gyn);
    else st3_bwd_point<DIMG, DCOORD, SRC>(b, di, g, H, W, xs, ys, gxn, gyn);
}

// ---------------------------------------------------------------------------------
// Backward of XS_HOMOG (warp.transformImage / transformCropImage / warpImage): what TensorFlow's autodiff gives for warp.py:46-86 and
// 89-129.  The coordinates and taps are homog_coords / homog_taps, the forward's, so every floor, ceil and inside decision is shared.
// floor, ceil and to_int32 have zero derivative and there is no clip: with xr = xw - floor(xw), yr likewise, per channel
//   d out / d xw = (UR - UL) (1 - yr) + (BR - BL) yr,   d out / d yw = (BL - UL) (1 - xr) + (BR - UR) xr,   a tap outside reading 0.
// Where xw is an exact integer floor == ceil, so UL == UR and the x slope is 0: the reference's behaviour, kept.
//   d img   the gather's adjoint: (1-xr)(1-yr), xr(1-yr), (1-xr)yr, xr yr times dout added to the four taps by float atomics, nothing
//           for a tap outside; with floor == ceil two taps of one address both add, as the reference's gather gradient does.
//   d M     [B,9]: gx, gy = the channel-summed slopes times dout; d xh = gx / zs, d yh = gy / zs, d zh = -(gx xh + gy yh) / zs^2, the
//           nine products with (X, Y, 1) in double from the forward's fp32 xh, yh, zs, X, Y; summed like d theta (part[workgroup][9],
//           st_theta_final_kernel<9>).  Composed form (ref given): M = ref . pM by compose3 as in the forward, and the final kernel
//           stores d pM = ref^T . d M.  A pixel none of whose taps is inside (a non-finite xw, yw among them) contributes nothing.
// ---------------------------------------------------------------------------------
__device__ __forceinline__ void homog_slope(const Taps &t, float UL, float UR, float BL, float BR, float g, float &gx, float &gy)
{
    const float xr = t.w0, yr = t.w1;
    gx = gx + ((UR - UL) * (1.0f - yr) + (BR - BL) * yr) * g;
    gy = gy + ((BL - UL) * (1.0f - xr) + (BR - UR) * xr) * g;
}

__device__ __forceinline__ void homog_accum(double *acc, float gxf, float gyf, const HomogPt &q)
{
    if (gxf == 0.0f && gyf == 0.0f) return;
    const double iz = 1.0 / (double)q.zs;
    const double gz = -((double)gxf * (double)q.xh + (double)gyf * (double)q.yh) * iz * iz;
    const double gx = (double)gxf * iz, gy = (double)gyf * iz;
    acc[0] += gx * (double)q.X; acc[1] += gx * (double)q.Y; acc[2] += gx;
    acc[3] += gy * (double)q.X; acc[4] += gy * (double)q.Y; acc[5] += gy;
    acc[6] += gz * (double)q.X; acc[7] += gz * (double)q.Y; acc[8] += gz;
}

// one output pixel, any channel count; gx, gy = d out / d (xw, yw) summed over the channels times dout (0 without DCOORD)
template <bool DIMG, bool DCOORD>
__device__ __forceinline__ void homog_bwd_point(const float *__restrict__ b, float *di, const float *__restrict__ g, int W, int C, const Taps &t,
                                                float &gx, float &gy)
{
    gx = gy = 0.0f;
    const bool v00 = t.vxa && t.vya, v01 = t.vxb && t.vya, v10 = t.vxa && t.vyb, v11 = t.vxb && t.vyb;
    if (!(v00 || v01 || v10 || v11)) return;
    const long long i00 = ((long long)t.ya * W + t.xa) * C, i01 = ((long long)t.ya * W + t.xb) * C;
    const long long i10 = ((long long)t.yb * W + t.xa) * C, i11 = ((long long)t.yb * W + t.xb) * C;
    const float xr = t.w0, yr = t.w1;
    const float w00 = (1.0f - xr) * (1.0f - yr), w01 = xr * (1.0f - yr), w10 = (1.0f - xr) * yr, w11 = xr * yr;
    for (int c = 0; c < C; ++c) {
        const float gc = g[c];
        if (DCOORD) homog_slope(t, v00 ? b[i00 + c] : 0.f, v01 ? b[i01 + c] : 0.f, v10 ? b[i10 + c] : 0.f, v11 ? b[i11 + c] : 0.f, gc, gx, gy);
        if (DIMG) {
            if (v00) atomicAdd(di + i00 + c, w00 * gc);
            if (v01) atomicAdd(di + i01 + c, w01 * gc);
            if (v10) atomicAdd(di + i10 + c, w10 * gc);
            if (v11) atomicAdd(di + i11 + c, w11 * gc);
        }
    }
}

// 3-channel frames (3 H W < 2^31: host)
template <bool DIMG, bool DCOORD>
__device__ __forceinline__ void homog3_bwd_point(const rgb3 *b, float *di, const rgb3 g, int W, const Taps &t, float &gx, float &gy)
{
    gx = gy = 0.0f;
    const bool v00 = t.vxa && t.vya, v01 = t.vxb && t.vya, v10 = t.vxa && t.vyb, v11 = t.vxb && t.vyb;
    if (!(v00 || v01 || v10 || v11)) return;
    if (DCOORD) {
        const rgb3 z = {0.f, 0.f, 0.f};
        const rgb3 UL = v00 ? b[t.ya * W + t.xa] : z, UR = v01 ? b[t.ya * W + t.xb] : z;
        const rgb3 BL = v10 ? b[t.yb * W + t.xa] : z, BR = v11 ? b[t.yb * W + t.xb] : z;
        homog_slope(t, UL.r, UR.r, BL.r, BR.r, g.r, gx, gy);
        homog_slope(t, UL.g, UR.g, BL.g, BR.g, g.g, gx, gy);
        homog_slope(t, UL.b, UR.b, BL.b, BR.b, g.b, gx, gy);
    }
    if (DIMG) {
        const float xr = t.w0, yr = t.w1;
        auto add = [&](int y, int x, bool valid, float w) {
            if (!valid) return;
            float *q = di + ((long long)y * W + x) * 3;
            atomicAdd(q, w * g.r); atomicAdd(q + 1, w * g.g); atomicAdd(q + 2, w * g.b);
        };
        add(t.ya, t.xa, v00, (1.0f - xr) * (1.0f - yr)); add(t.ya, t.xb, v01, xr * (1.0f - yr));
        add(t.yb, t.xa, v10, (1.0f - xr) * yr); add(t.yb, t.xb, v11, xr * yr);
    }
}

// doubles per d theta / d M partial row: the theta and symmetric-pad sources' 8 (the affine kinds use six of them; the symmetric-pad
// projective M[8] is a constant), the homography's 9
template <int SRC>
constexpr int st_part_width() { return SRC == XS_HOMOG ? 9 : 8; }

// any channel count, one thread per pixel (st_pixel_kernel's layout); d img the plain way
template <int SRC, bool DIMG, bool DCOORD, int INTERP = XI_BILINEAR>
__global__ __launch_bounds__(256) void st_pixel_bwd_kernel(const float *__restrict__ img, int H, int W, int C, StSrc S, StBwd G, int FH, int FW, unsigned bps)
{
    constexpr int NP = st_part_width<SRC>();
    __shared__ double red[4][NP];
    __shared__ float sm[SRC == XS_SYM ? 8 : 1];          // XS_SYM: st_matrix_wg's six similarity entries
    const int n = (int)(blockIdx.x / bps);
    float th[9];
    st_matrix_wg<SRC>(S, n, th, SRC == XS_SYM ? sm : nullptr);
    const long long p = (long long)(blockIdx.x - (unsigned)n * bps) * 256 + threadIdx.x;
    const bool ok = p < (long long)FH * FW;
    double acc[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) acc[k] = 0.0;
    if (ok && SRC == XS_HOMOG) {
        const int fy = (int)(p / FW), fx = (int)(p - (long long)fy * FW);
        const HomogPt q = homog_coords(th, fx, fy, S.dsx, S.dsy);
        float gx, gy;
        homog_bwd_point<DIMG, DCOORD>(img + (long long)n * H * W * C, DIMG ? G.d_img + (long long)n * H * W * C : nullptr,
                                      G.dout + ((long long)n * FH * FW + p) * C, W, C, homog_taps(q, H, W), gx, gy);
        if (DCOORD) homog_accum(acc, gx, gy, q);
    } else if (ok && SRC == XS_SYM) {
        const int fy = (int)(p / FW), fx = (int)(p - (long long)fy * FW);
        int gx, gy;
        if (st_grid_pos<SRC>(S, fx, fy, gx, gy)) {          // a pixel the crop-or-pad pads contributes nothing: its dout is not read
            float xs, ys, xh, yh, zs, gxn, gyn;
            const float xt = st_grid_t(gx, S.sx), yt = st_grid_t(gy, S.sy);
            st_sym_coords(th, S.kind == 1, xt, yt, xh, yh, zs, xs, ys);
            st_point_bwd<DIMG, DCOORD, SRC, INTERP>(img + (long long)n * H * W * C, DIMG ? G.d_img + (long long)n * H * W * C : nullptr,
                                                    G.dout + ((long long)n * FH * FW + p) * C, H, W, C, xs, ys, gxn, gyn);
            if (DCOORD) st_theta_accum(acc, S.tdim, gxn, gyn, xt, yt, xh, yh, zs);          // S.tdim: 8 projective, 6 otherwise (host)
        }
    } else if (ok) {
        const int fy = (int)(p / FW), fx = (int)(p - (long long)fy * FW);
        float xs, ys, xh = 0.f, yh = 0.f, zs = 1.f;
        const float xt = st_grid_t(fx, S.sx), yt = st_grid_t(fy, S.sy);
        if (SRC == XS_THETA) st_theta_coords(th, S.tdim, xt, yt, xh, yh, zs, xs, ys);
        else st_coords<SRC>(S, th, nullptr, n, fx, fy, xs, ys);
        float gxn, gyn;
        st_point_bwd<DIMG, DCOORD, XS_THETA, INTERP>(img + (long long)n * H * W * C, DIMG ? G.d_img + (long long)n * H * W * C : nullptr,
                                                     G.dout + ((long long)n * FH * FW + p) * C, H, W, C, xs, ys, gxn, gyn);
        if (DCOORD) {
            if (SRC == XS_COORDS) {
                if (G.d_x) G.d_x[(long long)n * FH * FW + p] = gxn;
                if (G.d_y) G.d_y[(long long)n * FH * FW + p] = gyn;
            } else {
                st_theta_accum(acc, S.tdim, gxn, gyn, xt, yt, xh, yh, zs);
            }
        }
    }
    if (DCOORD && (SRC == XS_THETA || SRC == XS_HOMOG || SRC == XS_SYM)) st_theta_reduce<NP>(acc, red, G.part + (long long)blockIdx.x * NP);
}

// 3-channel frames on the tile skeleton (st3_tile_kernel's pixels: a wave instruction works on a 4 x 16 patch)
template <int SRC, bool DIMG, bool DCOORD, int INTERP = XI_BILINEAR>
__global__ __launch_bounds__(256) void st3_tile_bwd_kernel(const float *__restrict__ img, int H, int W, StSrc S, StBwd G, int FH, int FW,
                                                           int tiles_x, int tiles_y)
{
    constexpr int PPT = StTile::PPT, NP = st_part_width<SRC>();
    __shared__ double red[4][NP];
    __shared__ float sm[SRC == XS_SYM ? 8 : 1];          // XS_SYM: st_matrix_wg's six similarity entries
    const StTile tile(tiles_x, tiles_y);
    const int n = tile.n;
    float th[9];
    st_matrix_wg<SRC>(S, n, th, SRC == XS_SYM ? sm : nullptr);
    const rgb3 *b = reinterpret_cast<const rgb3 *>(img) + (long long)n * H * W;     // 3 B H W < 2^31 (host)
    float *di = DIMG ? G.d_img + (long long)n * H * W * 3 : nullptr;
    double acc[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) acc[k] = 0.0;
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
        if (!(tile.y(j) < FH && tile.x(j) < FW)) continue;
        const int fy = tile.y(j), fx = tile.x(j);
        if (SRC == XS_HOMOG) {
            const HomogPt q = homog_coords(th, fx, fy, S.dsx, S.dsy);
            float gx, gy;
            homog3_bwd_point<DIMG, DCOORD>(b, di, reinterpret_cast<const rgb3 *>(G.dout)[((long long)n * FH + fy) * FW + fx], W, homog_taps(q, H, W), gx, gy);
            if (DCOORD) homog_accum(acc, gx, gy, q);
            continue;
        }
        if (SRC == XS_SYM) {
            int gx, gy;
            if (!st_grid_pos<SRC>(S, fx, fy, gx, gy)) continue;          // a pixel the crop-or-pad pads contributes nothing: its dout is not read
            float xs, ys, xh, yh, zs, gxn, gyn;
            const float xt = st_grid_t(gx, S.sx), yt = st_grid_t(gy, S.sy);
            st_sym_coords(th, S.kind == 1, xt, yt, xh, yh, zs, xs, ys);
            st3_point_bwd<DIMG, DCOORD, SRC, INTERP>(b, di, reinterpret_cast<const rgb3 *>(G.dout)[((long long)n * FH + fy) * FW + fx], H, W, xs, ys, gxn, gyn);
            if (DCOORD) st_theta_accum(acc, S.tdim, gxn, gyn, xt, yt, xh, yh, zs);          // S.tdim: 8 projective, 6 otherwise (host)
            continue;
        }
        float xs, ys, xh = 0.f, yh = 0.f, zs = 1.f;
        const float xt = st_grid_t(fx, S.sx), yt = st_grid_t(fy, S.sy);
        if (SRC == XS_THETA) st_theta_coords(th, S.tdim, xt, yt, xh, yh, zs, xs, ys);
        else st_coords<SRC>(S, th, nullptr, n, fx, fy, xs, ys);
        const long long po = ((long long)n * FH + fy) * FW + fx;
        float gxn, gyn;
        st3_point_bwd<DIMG, DCOORD, XS_THETA, INTERP>(b, di, reinterpret_cast<const rgb3 *>(G.dout)[po], H, W, xs, ys, gxn, gyn);
        if (DCOORD) {
            if (SRC == XS_COORDS) {
                if (G.d_x) G.d_x[po] = gxn;
                if (G.d_y) G.d_y[po] = gyn;
            } else {
                st_theta_accum(acc, S.tdim, gxn, gyn, xt, yt, xh, yh, zs);
            }
        }
    }
    if (DCOORD && (SRC == XS_THETA || SRC == XS_HOMOG || SRC == XS_SYM)) {
        const int tidx = (tile.ty0 / StTile::TH) * tiles_x + tile.tx0 / StTile::TW;
        st_theta_reduce<NP>(acc, red, G.part + ((long long)n * tiles_x * tiles_y + tidx) * NP);
    }
}

// workgroups per sample of the backward launch of this shape (the d theta partials are [B * workgroups][8] doubles), and whether it
// is the tile kernel's
static bool st_bwd_plan(int B, int H, int W, int C, int FH, int FW, int &tx, int &ty, dim3 &grid, long long &wgs)
{
    if (C == 3 && StTile::plan(B, FH, FW, 3 * std::max((long long)B * H * W, (long long)B * FH * FW), tx, ty, grid)) {
        wgs = (long long)tx * ty;
        return true;
    }
    wgs = ((long long)FH * FW + 255) / 256;
    return false;
}

size_t st_transform_backward_ws_bytes(int B, int H, int W, int C, int oh, int ow)
{
    int tx, ty;
    dim3 grid;
    long long wgs;
    st_bwd_plan(B, H, W, C, oh, ow, tx, ty, grid, wgs);
    return (size_t)wgs * B * 8 * sizeof(double);
}

template <int SRC, int INTERP = XI_BILINEAR>
static hipError_t launch_st_bwd(const float *img, int B, int H, int W, int C, StSrc S, StBwd G, int FH, int FW, hipStream_t stream)
{
    S.B = B;
    st_steps(S);
    if (SRC == XS_HOMOG) { S.dsx = S.gw > 1 ? 2.0 / (double)(S.gw - 1) : 0.0; S.dsy = S.gh > 1 ? 2.0 / (double)(S.gh - 1) : 0.0; }      // launch_st's
    const bool dimg = G.d_img != nullptr, dcoord = (SRC == XS_THETA || SRC == XS_HOMOG || SRC == XS_SYM) ? G.part != nullptr : (G.d_x || G.d_y);
    int tx, ty;
    dim3 grid;
    long long wgs;
    if (st_bwd_plan(B, H, W, C, FH, FW, tx, ty, grid, wgs)) {
#define ST_BWD_TILE(D, K) st3_tile_bwd_kernel<SRC, D, K, INTERP><<<grid, dim3(256), 0, stream>>>(img, H, W, S, G, FH, FW, tx, ty)
        if (dimg && dcoord) ST_BWD_TILE(true, true);
        else if (dimg) ST_BWD_TILE(true, false);
        else ST_BWD_TILE(false, true);
#undef ST_BWD_TILE
        return hipGetLastError();
    }
    if (wgs * B >= (1ll << 31)) return hipErrorInvalidValue;
    const dim3 pgrid((unsigned)(wgs * B));
#define ST_BWD_PIXEL(D, K) st_pixel_bwd_kernel<SRC, D, K, INTERP><<<pgrid, dim3(256), 0, stream>>>(img, H, W, C, S, G, FH, FW, (unsigned)wgs)
    if (dimg && dcoord) ST_BWD_PIXEL(true, true);
    else if (dimg) ST_BWD_PIXEL(true, false);
    else ST_BWD_PIXEL(false, true);
#undef ST_BWD_PIXEL
    return hipGetLastError();
}

hipError_t launch_st_transform_backward(const float *img, int B, int H, int W, int C, const float *theta, int tdim, const float *dout, int oh,
                                        int ow, float *d_img, int accumulate, float *d_theta, double *part, hipStream_t stream, int interp)
{
    if (d_img && !accumulate) {
        const hipError_t e = hipMemsetAsync(d_img, 0, (size_t)B * H * W * C * sizeof(float), stream);
        if (e != hipSuccess) return e;
    }
    StSrc S = st_plain(oh, ow);
    S.theta = theta; S.tdim = tdim;
    StBwd G{dout, d_img, nullptr, nullptr, d_theta ? part : nullptr};
    const hipError_t e = interp == XI_BICUBIC ? launch_st_bwd<XS_THETA, XI_BICUBIC>(img, B, H, W, C, S, G, oh, ow, stream)
                                              : launch_st_bwd<XS_THETA>(img, B, H, W, C, S, G, oh, ow, stream);
    if (e != hipSuccess || !d_theta) return e;
    int tx, ty;
    dim3 grid;
    long long wgs;
    st_bwd_plan(B, H, W, C, oh, ow, tx, ty, grid, wgs);
    st_theta_final_kernel<8><<<dim3((unsigned)B), dim3(256), 0, stream>>>(part, (int)wgs, tdim, d_theta);
    return hipGetLastError();
}

hipError_t launch_st_interp_backward(const float *img, int B, int H, int W, int C, const float *x, const float *y, const float *dout, int oh,
                                     int ow, float *d_img, int accumulate, float *d_x, float *d_y, hipStream_t stream, int interp)
{
    if (d_img && !accumulate) {
        const hipError_t e = hipMemsetAsync(d_img, 0, (size_t)B * H * W * C * sizeof(float), stream);
        if (e != hipSuccess) return e;
    }
    StSrc S = st_plain(oh, ow);
    S.x = x; S.y = y;
    StBwd G{dout, d_img, d_x, d_y, nullptr};
    if (interp == XI_BICUBIC) return launch_st_bwd<XS_COORDS, XI_BICUBIC>(img, B, H, W, C, S, G, oh, ow, stream);
    return launch_st_bwd<XS_COORDS>(img, B, H, W, C, S, G, oh, ow, stream);
}

// ---------------------------------------------------------------------------------
// Backward of the symmetric-pad transformers (XS_SYM, BILINEAR sampler): what TensorFlow's autodiff gives for ST:311-371, 454-517 and
// 611-716.  The two kernels above with SRC = XS_SYM: a final pixel goes through st_grid_pos (one the crop-or-pad pads contributes
// nothing), its coordinates are st_sym_coords', its axes those of the padded extent, and a padded tap p adds into image pixel
// refl(p - 100) -- the adjoint of gather . symmetric-pad.  The per-pixel products give d M, the gradient of the PRE-MAPPED matrix
// (part[workgroup][8], the projective kind's chain through x_h / z with z as is: no safe_z, z == 0 propagates by IEEE rules);
// st_sym_dm_kernel adds a sample's partials in st_theta_final_kernel's order into d M [B][8] doubles (behind the partials in the
// workspace), and st_sym_theta_final_kernel takes d M through the pre-map, in double, rounded to fp32 once:
//   affine      M = (theta c) 0 + I:  d theta[k] = (d M[k] 0) c[k] -- zero for a finite d M, a non-finite one propagates
//   projective  M = [theta, 1] P + A: d theta[k] = d M[k] P[k], k < 8
//   similarity  entry k of sample n is vector v = (6n+k) / B at batch index b = (6n+k) % B (st_matrix), so dE[v][b] = d M[n][k], and with
//               the forward's fp32 a, s, cosf a, sinf a:  d a = s (-sin a) (dE0 + dE4) + s cos a (dE1 - dE3),
//               d s = cos a (dE0 + dE4) + sin a (dE1 - dE3),  d theta[b] = (d a (float)(3.14/6), d s .1, dE2 .2, dE5 .2).
//               For B > 1 that couples samples: the kernel works on the whole batch, a thread per batch index.
// No atomics in either: d theta is bit-reproducible.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void st_sym_dm_kernel(const double *__restrict__ part, int wgs, double *__restrict__ dM)
{
    __shared__ double red[4][8];
    const int n = blockIdx.x;
    double acc[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = 0.0;
    for (int i = threadIdx.x; i < wgs; i += 256)
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] += part[((long long)n * wgs + i) * 8 + k];
    st_theta_reduce<8>(acc, red, dM + (long long)n * 8);
}

__global__ __launch_bounds__(64) void st_sym_theta_final_kernel(const double *__restrict__ dM, const float *__restrict__ theta, int B, int kind,
                                                                float *__restrict__ d_theta)
{
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    if (kind == 0) {
        const float c[6] = {0.1f, 0.0f, 0.2f, 0.1f, 0.0f, 0.2f};
#pragma unroll
        for (int k = 0; k < 6; ++k) d_theta[(long long)b * 6 + k] = (float)((dM[(long long)b * 8 + k] * 0.0) * (double)c[k]);
    } else if (kind == 1) {
        const float P[8] = {0.01f, 0.005f, 0.01f, 0.01f, 0.005f, 0.01f, 0.01f, 0.01f};
#pragma unroll
        for (int k = 0; k < 8; ++k) d_theta[(long long)b * 8 + k] = (float)(dM[(long long)b * 8 + k] * (double)P[k]);
    } else {
        double dE[6];
#pragma unroll
        for (int v = 0; v < 6; ++v) {                        // undo the interleave: (v, b) is entry k of sample n, 6n + k = v B + b
            const long long f = (long long)v * B + b;
            const long long n = f / 6;
            dE[v] = dM[n * 8 + (f - 6 * n)];
        }
        const float *tp = theta + (long long)b * 4;
        const float a = tp[0] * (float)(3.14 / 6) + 0.0f, s = tp[1] * 0.1f + 1.0f;          // st_matrix's
        const double ca = (double)cosf(a), sa = (double)sinf(a), sd = (double)s;
        const double d_a = sd * (-sa) * (dE[0] + dE[4]) + sd * ca * (dE[1] - dE[3]);
        const double d_s = ca * (dE[0] + dE[4]) + sa * (dE[1] - dE[3]);
        d_theta[(long long)b * 4 + 0] = (float)(d_a * (double)(float)(3.14 / 6));
        d_theta[(long long)b * 4 + 1] = (float)(d_s * (double)0.1f);
        d_theta[(long long)b * 4 + 2] = (float)(dE[2] * (double)0.2f);
        d_theta[(long long)b * 4 + 3] = (float)(dE[5] * (double)0.2f);
    }
}

// the partials [B * workgroups][8] and, behind them, d M [B][8]
size_t st_symmetry_backward_ws_bytes(int B, int H, int W, int C, int oh, int ow)
{
    int tx, ty;
    dim3 grid;
    long long wgs;
    st_bwd_plan(B, H, W, C, ow, oh, tx, ty, grid, wgs);          // the final extent: height ow, width oh
    return ((size_t)wgs * B * 8 + (size_t)B * 8) * sizeof(double);
}

hipError_t launch_st_symmetry_transform_backward(const float *img, int B, int H, int W, int C, const float *theta, int kind, const float *dout,
                                                 int oh, int ow, float *d_img, int accumulate, float *d_theta, double *part, hipStream_t stream,
                                                 int interp)
{
    if (d_img && !accumulate) {
        const hipError_t e = hipMemsetAsync(d_img, 0, (size_t)B * H * W * C * sizeof(float), stream);
        if (e != hipSuccess) return e;
    }
    int th, tw;
    const StSrc S = st_sym_src(theta, kind, oh, ow, th, tw);
    StBwd G{dout, d_img, nullptr, nullptr, d_theta ? part : nullptr};
    const hipError_t e = interp == XI_BICUBIC ? launch_st_bwd<XS_SYM, XI_BICUBIC>(img, B, H, W, C, S, G, th, tw, stream)
                                              : launch_st_bwd<XS_SYM>(img, B, H, W, C, S, G, th, tw, stream);
    if (e != hipSuccess || !d_theta) return e;
    int tx, ty;
    dim3 grid;
    long long wgs;
    st_bwd_plan(B, H, W, C, th, tw, tx, ty, grid, wgs);
    double *dM = part + wgs * B * 8;
    st_sym_dm_kernel<<<dim3((unsigned)B), dim3(256), 0, stream>>>(part, (int)wgs, dM);
    st_sym_theta_final_kernel<<<dim3((unsigned)((B + 63) / 64)), dim3(64), 0, stream>>>(dM, theta, B, kind, d_theta);
    return hipGetLastError();
}

size_t homography_warp_backward_ws_bytes(int B, int H, int W, int C, int oh, int ow)
{
    int tx, ty;
    dim3 grid;
    long long wgs;
    st_bwd_plan(B, H, W, C, oh, ow, tx, ty, grid, wgs);
    return (size_t)wgs * B * 9 * sizeof(double);
}

// ref == null: M [B,9] is the matrix and d_M its gradient; ref given: M holds pMtrx, the kernels compose ref . pMtrx as the forward
// does, and d_M receives d pMtrx = ref^T . d (ref . pMtrx)
hipError_t launch_homography_warp_backward(const float *img, int B, int Hi, int Wi, int C, const float *M, const float *ref, const float *dout,
                                           int oh, int ow, float *d_img, int accumulate, float *d_M, double *part, hipStream_t stream)
{
    if (d_img && !accumulate) {
        const hipError_t e = hipMemsetAsync(d_img, 0, (size_t)B * Hi * Wi * C * sizeof(float), stream);
        if (e != hipSuccess) return e;
    }
    StSrc S = st_plain(oh, ow);
    S.theta = M; S.tdim = 9; S.ref = ref;
    StBwd G{dout, d_img, nullptr, nullptr, d_M ? part : nullptr};
    const hipError_t e = launch_st_bwd<XS_HOMOG>(img, B, Hi, Wi, C, S, G, oh, ow, stream);
    if (e != hipSuccess || !d_M) return e;
    int tx, ty;
    dim3 grid;
    long long wgs;
    st_bwd_plan(B, Hi, Wi, C, oh, ow, tx, ty, grid, wgs);
    st_theta_final_kernel<9><<<dim3((unsigned)B), dim3(256), 0, stream>>>(part, (int)wgs, 9, d_M, ref);
    return hipGetLastError();
}

// Backward of vec2mtrx_kernel: d p [B,8|6] from d P [B,9].  The forward's recurrence N_i = N_{i-1} A, P += N_i / i! reversed:
// G_i = dP / i! + G_{i+1} A^T, d A += N_{i-1}^T G_i, which is d A = sum_i 1/i! sum_{j<i} (A^j)^T dP (A^{i-1-j})^T; then d A back through
// the generator layout (warp.py:28-33).  One thread per sample, in double from the fp32 p (the powers of A kept in a local array:
// approx <= 64 on the host), rounded to fp32 once.
constexpr int VEC2MTRX_MAX_APPROX = 64;

__device__ __forceinline__ void mat3_mul(const double *a, const double *b, double *o)
{
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) o[r * 3 + c] = (a[r * 3] * b[c] + a[r * 3 + 1] * b[3 + c]) + a[r * 3 + 2] * b[6 + c];
}

__global__ void vec2mtrx_bwd_kernel(const float *__restrict__ p, int B, int dim, int approx, const float *__restrict__ d_out, float *__restrict__ d_p)
{
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= B) return;
    const float *q = p + (long long)n * dim;
    double A[9], At[9], dP[9];
    if (dim == 8) {
        A[0] = (double)q[2]; A[1] = (double)q[1]; A[2] = (double)q[0];
        A[3] = (double)q[5]; A[4] = -(double)q[2] - (double)q[6]; A[5] = (double)q[4];
        A[6] = (double)q[3]; A[7] = (double)q[7]; A[8] = (double)q[6];
    } else {
        for (int k = 0; k < 6; ++k) A[k] = (double)q[k];
        A[6] = A[7] = A[8] = 0.0;
    }
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) At[r * 3 + c] = A[c * 3 + r];
    for (int k = 0; k < 9; ++k) dP[k] = (double)d_out[(long long)n * 9 + k];
    double Nt[VEC2MTRX_MAX_APPROX][9];                   // Nt[i] = (A^i)^T
    double fact = 1.0;                                   // (approx - 1)!
    for (int k = 0; k < 9; ++k) Nt[0][k] = (k % 4 == 0) ? 1.0 : 0.0;
    for (int i = 1; i < approx; ++i) {
        if (i < approx - 1) mat3_mul(At, Nt[i - 1], Nt[i]);          // (N A)^T = A^T N^T
        fact *= (double)i;
    }
    double Gm[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, dA[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = approx - 1; i >= 1; --i) {
        double T[9];
        mat3_mul(Gm, At, T);
        for (int k = 0; k < 9; ++k) Gm[k] = dP[k] / fact + T[k];
        mat3_mul(Nt[i - 1], Gm, T);
        for (int k = 0; k < 9; ++k) dA[k] += T[k];
        fact /= (double)i;
    }
    float *o = d_p + (long long)n * dim;
    if (dim == 8) {
        o[0] = (float)dA[2]; o[1] = (float)dA[1]; o[2] = (float)(dA[0] - dA[4]); o[3] = (float)dA[6];
        o[4] = (float)dA[5]; o[5] = (float)dA[3]; o[6] = (float)(dA[8] - dA[4]); o[7] = (float)dA[7];
    } else {
        for (int k = 0; k < 6; ++k) o[k] = (float)dA[k];
    }
}

hipError_t launch_vec2mtrx_backward(const float *p, int B, int dim, int approx, const float *d_out, float *d_p, hipStream_t stream)
{
    if (approx < 1 || approx > VEC2MTRX_MAX_APPROX) return hipErrorInvalidValue;
    vec2mtrx_bwd_kernel<<<dim3((unsigned)((B + 63) / 64)), dim3(64), 0, stream>>>(p, B, dim, approx, d_out, d_p);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------
// Backward of ElasticTransformer.transform (thin-plate spline, BILINEAR sampler).  The coefficients go into LDS through st_tps_coeff
// and the coordinates come from st_coords<XS_TPS>, as in the forward, so every tap decision is the forward's; a pixel's d img
// scatter and its gxn, gyn are st_bwd_point / st3_bwd_point, as for the other sources.
//   d theta  U_k depends on the grid alone, so with R = [x_t, y_t, 1, U_1..U_K]: d cf[r][j] = sum over the pixels of g_r R_j, 2 (K + 3)
//            sums per sample, then d theta[n, r K + k] = sum_j d cf[r][j] linv_t[k][j].  Products and sums in double, fp32 once.
//   layout   K + 3 reaches 259, so there are no per-thread accumulator arrays and no partial row per tile: sample n is walked by `wps`
//            workgroups (st_tps_bwd_plan), workgroup w taking the steps (tiles, or runs of 256 pixels) [w T / wps, (w + 1) T / wps)
//            in order.  A step: every thread does its pixels and stages (gxn, gyn, x_t, y_t) in LDS; then thread t OWNS control
//            point t % K and slice t / K of the staged pixels (256 / K slices) and adds g_r U_k into two doubles of its own, U_k
//            evaluated again by st_tps_U from the staged x_t, y_t (the forward's bits).  A column's sum never crosses lanes until
//            the workgroup is done: the slices are then added in slice order through LDS.  The three affine columns go per pixel
//            into st_theta_accum's six doubles and through st_theta_reduce (shuffles, then the four waves in order).  One partial
//            row [6 + 2 K] per workgroup: (gx x_t, gx y_t, gx, gy x_t, gy y_t, gy), the K x columns, the K y columns.
//            st_tps_theta_final_kernel adds a sample's rows in row order and applies linv_t.  No atomics: bit-reproducible.
// ---------------------------------------------------------------------------------
constexpr int ST_TPS_WG_TOTAL = 1024, ST_TPS_WPS_MIN = 16;      // workgroups per sample: max(16, 1024 / B), at most one per step

struct StTpsBwd {
    const float *dout;             // [B, FH, FW, C]
    float *d_img;                  // [B, H, W, C], added to (null: not wanted)
    double *part;                  // [B * wps][6 + 2 K] (null: d theta not wanted)
    int wps;
};

template <int P>                   // P pixels per step
struct StTpsLds {
    float cf[2 * (ST_TPS_KMAX + 3) + 2 * ST_TPS_KMAX];          // st_tps_coeff: coefficients, control points
    f32x4 px[P];                                                 // a step's pixels: gxn, gyn, x_t, y_t (identical addresses broadcast)
    double col[2][256], red[4][6];
};

// the staged pixels' share of this thread's column: control point k = t % K, pixels sl, sl + nsl, ... for slice sl = t / K
template <int P>
__device__ __forceinline__ void st_tps_columns(const f32x4 *px, const float *cf, int K, double &ax, double &ay)
{
    const int nsl = 256 / K, k = (int)threadIdx.x % K, sl = (int)threadIdx.x / K;
    if (sl >= nsl) return;
    const float cx = cf[2 * (K + 3) + k], cy = cf[2 * (K + 3) + K + k];
    for (int p = sl; p < P; p += nsl) {
        const f32x4 v = px[p];
        if (v.x == 0.0f && v.y == 0.0f) continue;                // outside the clip, or beyond the output
        const double U = (double)st_tps_U(v.z, v.w, cx, cy);
        ax += (double)v.x * U;
        ay += (double)v.y * U;
    }
}

// a workgroup's sums -> its partial row
template <int P>
__device__ __forceinline__ void st_tps_part(StTpsLds<P> &L, double *acc, double ax, double ay, int K, double *__restrict__ row)
{
    st_theta_reduce<6>(acc, L.red, row);
    L.col[0][threadIdx.x] = ax; L.col[1][threadIdx.x] = ay;      // a thread without a slice holds zeros
    __syncthreads();
    if ((int)threadIdx.x < K) {
        double sx = 0.0, sy = 0.0;
        for (int sl = 0; sl < 256 / K; ++sl) { sx += L.col[0][sl * K + threadIdx.x]; sy += L.col[1][sl * K + threadIdx.x]; }
        row[6 + threadIdx.x] = sx; row[6 + K + threadIdx.x] = sy;
    }
}

// any channel count: a step is a run of 256 pixels, one per thread
template <bool DIMG, bool DTHETA, int INTERP = XI_BILINEAR>
__global__ __launch_bounds__(256) void st_pixel_tps_bwd_kernel(const float *__restrict__ img, int H, int W, int C, StSrc S, StTpsBwd G, int FH, int FW,
                                                               int steps)
{
    __shared__ StTpsLds<256> L;
    const int n = (int)blockIdx.x / G.wps, w = (int)blockIdx.x - n * G.wps, K = S.g * S.g;
    st_tps_coeff(S, n, L.cf);
    __syncthreads();
    const int s0 = (int)((long long)w * steps / G.wps), s1 = (int)((long long)(w + 1) * steps / G.wps);
    double acc[6] = {0, 0, 0, 0, 0, 0}, ax = 0.0, ay = 0.0;
    for (int s = s0; s < s1; ++s) {
        const long long p = (long long)s * 256 + threadIdx.x;
        float gxn = 0.f, gyn = 0.f, xt = 0.f, yt = 0.f;
        if (p < (long long)FH * FW) {
            const int fy = (int)(p / FW), fx = (int)(p - (long long)fy * FW);
            xt = st_grid_t(fx, S.sx); yt = st_grid_t(fy, S.sy);
            float xs, ys;
            st_coords<XS_TPS>(S, nullptr, L.cf, n, fx, fy, xs, ys);
            st_point_bwd<DIMG, DTHETA, XS_TPS, INTERP>(img + (long long)n * H * W * C, DIMG ? G.d_img + (long long)n * H * W * C : nullptr,
                                                       G.dout + ((long long)n * FH * FW + p) * C, H, W, C, xs, ys, gxn, gyn);
            if (DTHETA) st_theta_accum(acc, 6, gxn, gyn, xt, yt, 0.f, 0.f, 1.f);
        }
        if (DTHETA) {
            L.px[threadIdx.x] = f32x4{gxn, gyn, xt, yt};
            __syncthreads();
            st_tps_columns<256>(L.px, L.cf, K, ax, ay);
            __syncthreads();
        }
    }
    if (DTHETA) st_tps_part(L, acc, ax, ay, K, G.part + (long long)blockIdx.x * (6 + 2 * K));
}

// 3-channel frames: a step is a tile of the tile skeleton (a wave instruction works on a 4 x 16 patch)
template <bool DIMG, bool DTHETA, int INTERP = XI_BILINEAR>
__global__ __launch_bounds__(256) void st3_tile_tps_bwd_kernel(const float *__restrict__ img, int H, int W, StSrc S, StTpsBwd G, int FH, int FW,
                                                               int tiles_x, int tiles_y)
{
    constexpr int PPT = StTile::PPT, P = StTile::TH * StTile::TW;
    __shared__ StTpsLds<P> L;
    const int n = (int)blockIdx.x / G.wps, w = (int)blockIdx.x - n * G.wps, K = S.g * S.g, steps = tiles_x * tiles_y;
    st_tps_coeff(S, n, L.cf);
    __syncthreads();
    StTile tile(tiles_x, tiles_y, false);
    const rgb3 *b = reinterpret_cast<const rgb3 *>(img) + (long long)n * H * W;     // 3 B H W < 2^31 (host)
    float *di = DIMG ? G.d_img + (long long)n * H * W * 3 : nullptr;
    const int s0 = (int)((long long)w * steps / G.wps), s1 = (int)((long long)(w + 1) * steps / G.wps);
    double acc[6] = {0, 0, 0, 0, 0, 0}, ax = 0.0, ay = 0.0;
    for (int s = s0; s < s1; ++s) {
        tile.seat(n, s, tiles_x);
#pragma unroll
        for (int j = 0; j < PPT; ++j) {
            float gxn = 0.f, gyn = 0.f, xt = 0.f, yt = 0.f;
            if (tile.y(j) < FH && tile.x(j) < FW) {
                const int fy = tile.y(j), fx = tile.x(j);
                xt = st_grid_t(fx, S.sx); yt = st_grid_t(fy, S.sy);
                float xs, ys;
                st_coords<XS_TPS>(S, nullptr, L.cf, n, fx, fy, xs, ys);
                const long long po = ((long long)n * FH + fy) * FW + fx;
                st3_point_bwd<DIMG, DTHETA, XS_TPS, INTERP>(b, di, reinterpret_cast<const rgb3 *>(G.dout)[po], H, W, xs, ys, gxn, gyn);
                if (DTHETA) st_theta_accum(acc, 6, gxn, gyn, xt, yt, 0.f, 0.f, 1.f);
            }
            if (DTHETA) L.px[tile.staged(j)] = f32x4{gxn, gyn, xt, yt};
        }
        if (DTHETA) {
            __syncthreads();
            st_tps_columns<P>(L.px, L.cf, K, ax, ay);
            __syncthreads();
        }
    }
    if (DTHETA) st_tps_part(L, acc, ax, ay, K, G.part + (long long)blockIdx.x * (6 + 2 * K));
}

// d theta[n, r K + k] = sum_j d cf[r][j] linv_t[k][j] in double: sample n's `wps` partial rows added in row order, a thread per column,
// into LDS; then a thread per offset, the three affine products and the K others in j order; rounded to fp32 once
__global__ __launch_bounds__(256) void st_tps_theta_final_kernel(const double *__restrict__ part, int wps, int K, const float *__restrict__ linv_t,
                                                                 float *__restrict__ d_theta)
{
    __shared__ double dcf[6 + 2 * ST_TPS_KMAX];
    const int n = blockIdx.x, RW = 6 + 2 * K;
    for (int c = threadIdx.x; c < RW; c += 256) {
        double s = 0.0;
        for (int w = 0; w < wps; ++w) s += part[((long long)n * wps + w) * RW + c];
        dcf[c] = s;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < 2 * K; e += 256) {
        const int r = e / K, k = e - r * K;
        const float *lk = linv_t + (long long)k * (K + 3);
        double s = (dcf[3 * r] * (double)lk[0] + dcf[3 * r + 1] * (double)lk[1]) + dcf[3 * r + 2] * (double)lk[2];
        for (int j = 0; j < K; ++j) s += dcf[6 + r * K + j] * (double)lk[3 + j];
        d_theta[(long long)n * 2 * K + e] = (float)s;
    }
}

// the walking launch of this shape: steps per sample (st_bwd_plan's tiles, or runs of 256 pixels), workgroups per sample, and whether
// it is the tile kernel's
static bool st_tps_bwd_plan(int B, int H, int W, int C, int FH, int FW, int &tx, int &ty, long long &steps, int &wps)
{
    dim3 grid;
    const bool tiled = st_bwd_plan(B, H, W, C, FH, FW, tx, ty, grid, steps);
    wps = (int)std::min<long long>(steps, std::max(ST_TPS_WPS_MIN, ST_TPS_WG_TOTAL / B));
    return tiled;
}

// B * wps rows of 2 (K + 3) doubles with wps = min(steps, max(16, 1024 / B)): whatever the frame size, at most
// max(1024, 16 B) * 2 (K + 3) * 8 bytes -- 4 MiB at K = 256 up to B = 64
size_t st_elastic_backward_ws_bytes(int B, int H, int W, int C, int g, int oh, int ow)
{
    int tx, ty, wps;
    long long steps;
    st_tps_bwd_plan(B, H, W, C, oh, ow, tx, ty, steps, wps);
    return (size_t)B * wps * (6 + 2 * g * g) * sizeof(double);
}

hipError_t launch_st_elastic_transform_backward(const float *img, int B, int H, int W, int C, const float *theta, int g, const float *linv_t,
                                                const float *dout, int oh, int ow, float *d_img, int accumulate, float *d_theta, double *part,
                                                hipStream_t stream, int interp)
{
    if (d_img && !accumulate) {
        const hipError_t e = hipMemsetAsync(d_img, 0, (size_t)B * H * W * C * sizeof(float), stream);
        if (e != hipSuccess) return e;
    }
    const StSrc S = st_elastic_src(B, theta, g, linv_t, oh, ow);
    int tx, ty, wps;
    long long steps;
    const bool tiled = st_tps_bwd_plan(B, H, W, C, oh, ow, tx, ty, steps, wps);
    if (steps >= (1ll << 31)) return hipErrorInvalidValue;
    const StTpsBwd G{dout, d_img, d_theta ? part : nullptr, wps};
    const bool dimg = d_img != nullptr, dtheta = d_theta != nullptr;
    const dim3 grid((unsigned)((long long)B * wps));
    if (tiled) {
#define ST_TPS_TILE(D, T)                                                                                                            \
    do {                                                                                                                             \
        if (interp == XI_BICUBIC) st3_tile_tps_bwd_kernel<D, T, XI_BICUBIC><<<grid, dim3(256), 0, stream>>>(img, H, W, S, G, oh, ow, tx, ty); \
        else st3_tile_tps_bwd_kernel<D, T><<<grid, dim3(256), 0, stream>>>(img, H, W, S, G, oh, ow, tx, ty);                         \
    } while (0)
        if (dimg && dtheta) ST_TPS_TILE(true, true);
        else if (dimg) ST_TPS_TILE(true, false);
        else ST_TPS_TILE(false, true);
#undef ST_TPS_TILE
    } else {
#define ST_TPS_PIXEL(D, T)                                                                                                           \
    do {                                                                                                                             \
        if (interp == XI_BICUBIC) st_pixel_tps_bwd_kernel<D, T, XI_BICUBIC><<<grid, dim3(256), 0, stream>>>(img, H, W, C, S, G, oh, ow, (int)steps); \
        else st_pixel_tps_bwd_kernel<D, T><<<grid, dim3(256), 0, stream>>>(img, H, W, C, S, G, oh, ow, (int)steps);                  \
    } while (0)
        if (dimg && dtheta) ST_TPS_PIXEL(true, true);
        else if (dimg) ST_TPS_PIXEL(true, false);
        else ST_TPS_PIXEL(false, true);
#undef ST_TPS_PIXEL
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !dtheta) return e;
    st_tps_theta_final_kernel<<<dim3((unsigned)B), dim3(256), 0, stream>>>(part, wps, g * g, linv_t, d_theta);
    return hipGetLastError();
}

}  // namespace vstab
