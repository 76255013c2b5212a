// The per-axis arithmetic of the reference's bilinear samplers (spatial_transformer.py: bilinear_interp ST:902-964, one pixel of
// zero border; bilinear_interp3d ST:797-899, edge_size voxels of it) and the reproducible d theta reduction, stated once for the
// 2-D family (sampler_ops.hip) and the 3-D one (sampler3d_ops.hip).  Device code only.
#pragma once
#include "vstab_internal.h"

namespace vstab {

// tf.linspace(-1, 1, n)[i] in fp32 (start + i*step, step = 2/(n-1); a single point is -1)
__device__ __forceinline__ float lin11(int i, int n)
{
    const float step = n > 1 ? 2.0f / (float)(n - 1) : 0.0f;
    return -1.0f + (float)i * step;
}

// point i of the linspace(-1, 1) sampling grid whose step is `step` (2/(n-1), divided once on the host: the same IEEE quotient
// lin11 computes)
__device__ __forceinline__ float st_grid_t(int i, float step) { return -1.0f + (float)i * step; }

// One axis of bilinear_interp / bilinear_interp3d: v = (v+1)/2*(n-1), clipped to [-e, n-1+e], shifted by the e-pixel zero pad
// (e = 1 in 2-D); v0 = floor, v1 = min(v0+1, n-1+2e) as index but the weights use the UNclipped v0+1.
// lo = v - v0, hi = (v0+1) - v (both exact in fp32); a, b the two image indices clamped into the image (what is addressed), va, vb
// whether they count (a tap on the zero border reads as zero).  pass: the clip lets a gradient through, -e <= v <= n-1+e
// inclusive, not for NaN (the backward's rule).
struct Axis { float lo, hi; int a, b; bool va, vb, pass; };

__device__ __forceinline__ Axis st_axis(float vn, int n, int e = 1)
{
    const float nf = (float)n, ef = (float)e;
    float v = (vn + 1.0f) / 2.0f * (nf - 1.0f);
    Axis A;
    A.pass = v >= -ef && v <= nf - 1.0f + ef;
    v = fminf(fmaxf(v, -ef), nf - 1.0f + ef);            // clip_by_value(x, -edge, W-1+edge); NaN -> -edge
    v += ef;
    const float v0f = floorf(v), v1f = v0f + 1.0f;
    const int v0 = (int)v0f;                             // in [0, n-1+2e] after the clip
    const int v1 = (int)fminf(v1f, nf - 1.0f + (float)(2 * e));
    A.lo = v - v0f; A.hi = v1f - v;
    // padded index p in [0, n-1+2e]: image index p-e, zero on the border
    A.va = v0 >= e && v0 <= n - 1 + e; A.vb = v1 >= e && v1 <= n - 1 + e;
    A.a = min(max(v0 - e, 0), n - 1); A.b = min(max(v1 - e, 0), n - 1);
    return A;
}

// the clip's gradient rule and the chain through (v + 1) / 2 * (n - 1)
__device__ __forceinline__ float st_axis_chain(const Axis &A, float g, int n) { return A.pass ? g * (((float)n - 1.0f) / 2.0f) : 0.0f; }

// acc[K] of every thread of a 256-thread workgroup -> part[K]: xor-shuffles inside a wave, the four waves added in wave order
template <int K>
__device__ __forceinline__ void st_theta_reduce(double *acc, double (*red)[K], double *__restrict__ part)
{
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) acc[k] += __shfl_xor(acc[k], o, 64);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) red[wave][k] = acc[k];
    __syncthreads();
    if (threadIdx.x < K) part[threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// d theta[n, k] = sum of sample n's `wgs` partials [K]: thread t adds partials t, t + 256, ..., then st_theta_reduce's order.
// `left` (K = 9 only; null otherwise): the totals are a 3 x 3 matrix d M of M = left . P, and what is stored is d P = left^T . d M,
// the three products of an entry in double, (l0 d0 + l1 d1) + l2 d2, rounded to fp32 once.
template <int K>
__global__ __launch_bounds__(256) void st_theta_final_kernel(const double *__restrict__ part, int wgs, int tdim, float *__restrict__ d_theta,
                                                             const float *__restrict__ left = nullptr)
{
    __shared__ double red[4][K], tot[K];
    const int n = blockIdx.x;
    double acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.0;
    for (int i = threadIdx.x; i < wgs; i += 256)
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] += part[((long long)n * wgs + i) * K + k];
    st_theta_reduce<K>(acc, red, tot);
    __syncthreads();
    if (K == 9 && left) {
        if (threadIdx.x < 9) {
            const int i = threadIdx.x / 3, j = threadIdx.x - 3 * i;
            d_theta[(long long)n * 9 + threadIdx.x] =
                (float)(((double)left[i] * tot[j] + (double)left[3 + i] * tot[3 + j]) + (double)left[6 + i] * tot[6 + j]);
        }
        return;
    }
    if ((int)threadIdx.x < tdim) d_theta[(long long)n * tdim + threadIdx.x] = (float)tot[threadIdx.x];
}

}  // namespace vstab
