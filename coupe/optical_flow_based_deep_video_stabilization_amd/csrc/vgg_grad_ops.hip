// Backward pieces of the VGG16 trunk that the training convolutions do not cover: the fused backward of
// 2x2 SAME max-pool + the ReLU gate of the conv that fed it, the bare ReLU gate, and the 3-channel first layer's input and filter
// gradients.  All four are bandwidth-bound: each reads its operands once and writes its result once.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "vstab_internal.h"

namespace vstab {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---- max-pool (2, 2, SAME) backward fused with ReluGrad of its input.  y [B,H,W,C] is the post-ReLU conv output, dpool
// [B,ceil(H/2),ceil(W/2),C] the gradient at the pooled tensor.  One thread per 4 channels of one 2x2 input window: windows do not
// overlap (stride = kernel), so each element of dy has exactly one writer and no atomics are needed.
// Tie rule: the whole gradient goes to the FIRST maximum in the order (0,0), (0,1), (1,0), (1,1) among the taps inside the image
// (the taps beyond the bottom / right edge take no part, as in maxpool2x2_kernel).  ⚠ This is TensorFlow's MaxPoolGrad as recalled,
// not read from its source.  Zero rule: the gradient passes only where y > 0 (TF's ReluGrad), so a window whose maximum is 0
// passes nothing.  accumulate: dy already holds the caller's gradient at y; the result is (dy + routed) gated by y > 0.
__global__ __launch_bounds__(256) void maxpool2x2_relu_backward_kernel(const float *__restrict__ y, int B, int H, int W, int C4,
                                                                       const float *__restrict__ dpool, int oh, int ow,
                                                                       float *__restrict__ dy, int accumulate)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long total = (long long)B * oh * ow * C4;
    if (idx >= total) return;
    const int c = (int)(idx % C4);
    const long long pix = idx / C4;
    const int n = (int)(pix / (oh * ow));
    const int rem = (int)(pix - (long long)n * oh * ow);
    const int oy = rem / ow, ox = rem - oy * ow;
    const int y0 = 2 * oy, x0 = 2 * ox;
    const bool ok[4] = {true, x0 + 1 < W, y0 + 1 < H, x0 + 1 < W && y0 + 1 < H};
    const long long base = (long long)n * H * W * C4 + c;
    const long long off[4] = {base + ((long long)y0 * W + x0) * C4, base + ((long long)y0 * W + x0 + 1) * C4,
                              base + ((long long)(y0 + 1) * W + x0) * C4, base + ((long long)(y0 + 1) * W + x0 + 1) * C4};
    const f32x4 *yv = reinterpret_cast<const f32x4 *>(y);
    f32x4 *dv = reinterpret_cast<f32x4 *>(dy);
    const f32x4 g = reinterpret_cast<const f32x4 *>(dpool)[idx];
    f32x4 v[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) v[t] = ok[t] ? yv[off[t]] : f32x4{0.f, 0.f, 0.f, 0.f};
    int best[4] = {0, 0, 0, 0};
    f32x4 m = v[0];
#pragma unroll
    for (int t = 1; t < 4; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (ok[t] && v[t][e] > m[e]) { m[e] = v[t][e]; best[e] = t; }      // strictly greater: the first maximum keeps it
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        if (!ok[t]) continue;
        f32x4 r;
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] = (best[e] == t && v[t][e] > 0.f) ? g[e] : 0.f;
        if (accumulate) {
            const f32x4 old = dv[off[t]];
#pragma unroll
            for (int e = 0; e < 4; ++e) r[e] = v[t][e] > 0.f ? old[e] + r[e] : 0.f;
        }
        dv[off[t]] = r;
    }
}

hipError_t launch_maxpool2x2_relu_backward(const float *y, int B, int H, int W, int C, const float *dpool, float *dy, int accumulate,
                                           hipStream_t stream)
{
    if (B < 1 || H < 1 || W < 1 || C < 4 || (C & 3)) return hipErrorInvalidValue;
    const int oh = (H + 1) / 2, ow = (W + 1) / 2;
    const long long total = (long long)B * oh * ow * (C / 4);
    if ((total + 255) / 256 > 0x7fffffffLL) return hipErrorInvalidValue;
    maxpool2x2_relu_backward_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream>>>(y, B, H, W, C / 4, dpool, oh, ow, dy,
                                                                                                      accumulate ? 1 : 0);
    return hipGetLastError();
}

// ---- dy *= (y > 0) in place, n4 float4s: the gate of a conv output that feeds another conv directly
__global__ __launch_bounds__(256) void relu_backward_kernel(const f32x4 *__restrict__ y, f32x4 *__restrict__ dy, long long n4)
{
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
        const f32x4 v = y[i];
        f32x4 d = dy[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) d[e] = v[e] > 0.f ? d[e] : 0.f;
        dy[i] = d;
    }
}

hipError_t launch_relu_backward(const float *y, float *dy, long long n4, hipStream_t stream)
{
    if (n4 < 1) return hipErrorInvalidValue;
    const long long blocks = std::min<long long>((n4 + 255) / 256, 256 * 16);        // grid-stride above 16 workgroups per CU
    relu_backward_kernel<<<dim3((unsigned)blocks), dim3(256), 0, stream>>>(reinterpret_cast<const f32x4 *>(y), reinterpret_cast<f32x4 *>(dy), n4);
    return hipGetLastError();
}

// ---- conv1_1's input gradient: dx[n,y,x,ci] = sum over (ky,kx,co) of g[n, y-ky+1, x-kx+1, co] * W[ky,kx,ci,co].  The gradient it
// reads is the large tensor (cout floats per pixel against 3 written), so the kernel is shaped for that read: 16 lanes per pixel,
// one float4 of the cout channels each (one contiguous pixel row of g per tap; the nine taps of neighbouring pixels come through
// L1 / L2), the 27 x cout filter in LDS in the forward's layout, and a 16-lane butterfly that leaves the three sums in lane 0.
__global__ __launch_bounds__(256) void conv3x3_rgb_dgrad_kernel(const float *__restrict__ g, int B, int H, int W, const float *__restrict__ Wf,
                                                                int cout, float *__restrict__ dx)
{
    __shared__ f32x4 sW[27 * 16];
    const int q4 = cout >> 2;
    for (int i = threadIdx.x; i < 27 * 16; i += 256) {
        const int r = i >> 4, q = i & 15;
        sW[i] = q < q4 ? *reinterpret_cast<const f32x4 *>(Wf + (long long)r * cout + q * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    __syncthreads();
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const int q = (int)(idx & 15);
    const long long pix = idx >> 4;
    const bool live = pix < (long long)B * H * W;          // whole 16-lane groups are live or not; every lane takes part in the shuffles
    const long long pp = live ? pix : 0;
    const int n = (int)(pp / ((long long)H * W));
    const int rem = (int)(pp - (long long)n * H * W);
    const int py = rem / W, px = rem - py * W;
    const float *gb = g + (long long)n * H * W * cout + q * 4;
    float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        const int gy = py - ky + 1;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int gx = px - kx + 1;
            const bool ok = live && q < q4 && (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W;
            const f32x4 v = ok ? *reinterpret_cast<const f32x4 *>(gb + ((long long)gy * W + gx) * cout) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ci = 0; ci < 3; ++ci) {
                const f32x4 w = sW[((ky * 3 + kx) * 3 + ci) * 16 + q];
                acc[ci] += (v[0] * w[0] + v[1] * w[1]) + (v[2] * w[2] + v[3] * w[3]);
            }
        }
    }
#pragma unroll
    for (int ci = 0; ci < 3; ++ci)
#pragma unroll
        for (int m = 8; m >= 1; m >>= 1) acc[ci] += __shfl_xor(acc[ci], m, 16);
    if (live && q == 0) {
        float *o = dx + pix * 3;
        o[0] = acc[0]; o[1] = acc[1]; o[2] = acc[2];
    }
}

hipError_t launch_conv3x3_rgb_dgrad(const float *gout, int B, int H, int W, const float *Wf, int cout, float *dx, hipStream_t stream)
{
    if (B < 1 || H < 1 || W < 1 || (cout & 3) || cout > 64 || cout < 4) return hipErrorInvalidValue;
    const long long n = (long long)B * H * W * 16;
    if ((n + 255) / 256 > 0x7fffffffLL) return hipErrorInvalidValue;
    conv3x3_rgb_dgrad_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream>>>(gout, B, H, W, Wf, cout, dx);
    return hipGetLastError();
}

// ---- conv1_1's filter and bias gradient: dW[ky,kx,ci,co] = sum over pixels of x[n, y+ky-1, x+kx-1, ci] * g[n,y,x,co], db[co] = sum g.
// vstab_conv_wgrad refuses cin = 3 (its gathers are float4s of channels).  A reduction over every pixel into 28 x cout numbers: a
// workgroup is 16 pixel lanes x 16 float4s of cout, each thread keeps its 28 float4 sums in registers over a strided share of the
// pixels; the four pixel lanes of a wave fold by shuffle, the four waves through LDS, and each workgroup writes one [28][64] slab.
// A second launch adds the slabs in a fixed order (no atomics: the result does not depend on scheduling).
constexpr int RGB_WGRAD_ROWS = 28;                 // 27 filter rows + the bias row
constexpr int RGB_WGRAD_SLAB = RGB_WGRAD_ROWS * 64;

__global__ __launch_bounds__(256) void conv3x3_rgb_wgrad_kernel(const float *__restrict__ x, const float *__restrict__ g, int B, int H, int W,
                                                                int cout, float *__restrict__ slabs)
{
    __shared__ f32x4 sR[4][RGB_WGRAD_ROWS][16];
    const int q = threadIdx.x & 15, pl = threadIdx.x >> 4, q4 = cout >> 2;
    const long long npix = (long long)B * H * W;
    f32x4 acc[RGB_WGRAD_ROWS];
#pragma unroll
    for (int r = 0; r < RGB_WGRAD_ROWS; ++r) acc[r] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (long long p = (long long)blockIdx.x * 16 + pl; p < npix; p += (long long)gridDim.x * 16) {
        const int n = (int)(p / ((long long)H * W));
        const int rem = (int)(p - (long long)n * H * W);
        const int py = rem / W, px = rem - py * W;
        const f32x4 gv = q < q4 ? *reinterpret_cast<const f32x4 *>(g + p * cout + q * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
        const float *xb = x + (long long)n * H * W * 3;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = py + ky - 1;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int ix = px + kx - 1;
                const bool ok = (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
                const float *s = xb + ((long long)iy * W + ix) * 3;
#pragma unroll
                for (int ci = 0; ci < 3; ++ci) {
                    const float xv = ok ? s[ci] : 0.f;
                    acc[(ky * 3 + kx) * 3 + ci] += xv * gv;
                }
            }
        }
        acc[27] += gv;
    }
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int r = 0; r < RGB_WGRAD_ROWS; ++r) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float s = acc[r][e];
            s += __shfl_xor(s, 16, 64);
            s += __shfl_xor(s, 32, 64);
            acc[r][e] = s;
        }
        if ((threadIdx.x & 63) < 16) sR[wave][r][q] = acc[r];
    }
    __syncthreads();
    float *slab = slabs + (long long)blockIdx.x * RGB_WGRAD_SLAB;
    for (int i = threadIdx.x; i < RGB_WGRAD_ROWS * 16; i += 256) {
        const int r = i >> 4, c = i & 15;
        const f32x4 s = (sR[0][r][c] + sR[1][r][c]) + (sR[2][r][c] + sR[3][r][c]);
        *reinterpret_cast<f32x4 *>(slab + r * 64 + c * 4) = s;
    }
}

__global__ __launch_bounds__(256) void conv3x3_rgb_wgrad_fold_kernel(const float *__restrict__ slabs, int nslabs, int cout, float *__restrict__ dW,
                                                                     float *__restrict__ db, int accumulate)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= RGB_WGRAD_SLAB) return;
    const int r = i >> 6, c = i & 63;
    if (c >= cout) return;
    float s = 0.f;
    for (int k = 0; k < nslabs; ++k) s += slabs[(long long)k * RGB_WGRAD_SLAB + i];
    float *dst = r < 27 ? dW + r * cout + c : (db ? db + c : nullptr);
    if (dst) *dst = accumulate ? *dst + s : s;
}

int conv3x3_rgb_wgrad_slabs(long long npix)
{
    return (int)std::max<long long>(1, std::min<long long>((npix + 127) / 128, 512));      // >= 8 pixels per lane, two workgroups per CU
}

size_t conv3x3_rgb_wgrad_scratch_bytes(long long npix) { return (size_t)conv3x3_rgb_wgrad_slabs(npix) * RGB_WGRAD_SLAB * sizeof(float); }

hipError_t launch_conv3x3_rgb_wgrad(const float *x, const float *gout, int B, int H, int W, int cout, float *dW, float *db, int accumulate,
                                    float *scratch, hipStream_t stream)
{
    if (B < 1 || H < 1 || W < 1 || (cout & 3) || cout > 64 || cout < 4) return hipErrorInvalidValue;
    const int nslabs = conv3x3_rgb_wgrad_slabs((long long)B * H * W);
    conv3x3_rgb_wgrad_kernel<<<dim3(nslabs), dim3(256), 0, stream>>>(x, gout, B, H, W, cout, scratch);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    conv3x3_rgb_wgrad_fold_kernel<<<dim3((RGB_WGRAD_SLAB + 255) / 256), dim3(256), 0, stream>>>(scratch, nslabs, cout, dW, db, accumulate ? 1 : 0);
    return hipGetLastError();
}

}  // namespace vstab
