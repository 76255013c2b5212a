// Kernels of utils.py's image-similarity measures (utils.py:74-166): the structure term of SSIM over a separable Gaussian
// window, its gradient, and the 2x2 stride-2 SAME average pool of the multi-scale form.
//
//   mu1 = w*x, mu2 = w*y, s1 = w*x^2 - mu1^2, s2 = w*y^2 - mu2^2, s12 = w*xy - mu1 mu2   (five VALID k x k correlations)
//   s = (s12^2 + C3) / (s1 s2 + C3),  C3 = 0.03^2 / 2                                    (utils.py:111; l**0 and c**0 are 1)
//
// The window of _tf_fspecial_gauss is the outer product of a 1-D vector with itself (ssim_api.cpp makes that vector), so each
// correlation is a row pass followed by a column pass.  One workgroup of 256 threads owns a tile of 16 x 64 outputs: both images'
// (16+k-1) x (64+k-1) patch goes to LDS, the row pass leaves the five row sums of (16+k-1) x 64 positions in LDS, and in the column
// pass each thread walks 4 + k - 1 rows of one column for its 4 outputs.  k is a template argument (the host picks the instance for
// the run-time size 1..11), so every array is sized at compile time and the taps unroll with their weights in scalar registers.
// Sums are chains of fmaf in a fixed order; the per-sample mean is per-workgroup partial sums plus a second pass, no atomics:
// two runs give the same bits.
//
// Gradient, two launches (DESIGN.md says why not one): ssim_grad_fields_kernel recomputes the moments as the forward does and
// writes g * ds/d{mu1, mu2, E[x^2], E[y^2], E[xy]} as five planes; ssim_adjoint_kernel gathers them through the adjoint of the VALID
// correlation (the flipped window over the zero-extended planes) and combines  dx = A(g_mu1) + 2x A(g_xx) + y A(g_xy).
#include "vstab_internal.h"

namespace vstab {

namespace {

constexpr int TH = 16, TW = 64, ROWS = TH / 4;      // 256 threads: column tx = t & 63, rows (t >> 6) * 4 .. + 3
constexpr float SSIM_C3 = 0.03f * 0.03f / 2.0f;

template <int K> struct SsimSmem {
    static constexpr int RH = TH + K - 1, RW = TW + K - 1;
    float sx[RH * RW];
    float sy[RH * RW];
    float rp[5][RH * TW];
};

// the five windowed moments {mu1, mu2, E[x^2], E[y^2], E[xy]} of this thread's ROWS outputs of the tile at (i0, j0); x, y: one sample
template <int K>
__device__ __forceinline__ void ssim_tile_moments(const float *__restrict__ x, const float *__restrict__ y, int H, int W, int i0, int j0,
                                                  const SsimWindow &win, SsimSmem<K> &sm, float (&m)[ROWS][5])
{
    constexpr int RH = SsimSmem<K>::RH, RW = SsimSmem<K>::RW;
    const int t = threadIdx.x;
    for (int idx = t; idx < RH * RW; idx += 256) {
        const int r = idx / RW, c = idx - r * RW;
        const int gi = i0 + r, gj = j0 + c;
        const bool in = gi < H && gj < W;
        sm.sx[idx] = in ? x[gi * W + gj] : 0.f;
        sm.sy[idx] = in ? y[gi * W + gj] : 0.f;
    }
    __syncthreads();
    for (int idx = t; idx < RH * TW; idx += 256) {
        const int r = idx / TW, c = idx - r * TW;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f;
#pragma unroll
        for (int b = 0; b < K; ++b) {
            const float xv = sm.sx[r * RW + c + b], yv = sm.sy[r * RW + c + b], wb = win.w[b];
            a0 = fmaf(wb, xv, a0);
            a1 = fmaf(wb, yv, a1);
            a2 = fmaf(wb, xv * xv, a2);
            a3 = fmaf(wb, yv * yv, a3);
            a4 = fmaf(wb, xv * yv, a4);
        }
        sm.rp[0][idx] = a0; sm.rp[1][idx] = a1; sm.rp[2][idx] = a2; sm.rp[3][idx] = a3; sm.rp[4][idx] = a4;
    }
    __syncthreads();
    const int tx = t & 63, r0 = (t >> 6) * ROWS;
#pragma unroll
    for (int o = 0; o < ROWS; ++o)
#pragma unroll
        for (int f = 0; f < 5; ++f) m[o][f] = 0.f;
#pragma unroll
    for (int rr = 0; rr < ROWS + K - 1; ++rr) {
        float v[5];
#pragma unroll
        for (int f = 0; f < 5; ++f) v[f] = sm.rp[f][(r0 + rr) * TW + tx];
#pragma unroll
        for (int o = 0; o < ROWS; ++o) {
            const int a = rr - o;
            if (a >= 0 && a < K) {
#pragma unroll
                for (int f = 0; f < 5; ++f) m[o][f] = fmaf(win.w[a], v[f], m[o][f]);
            }
        }
    }
}

struct SsimTerms { float s1, s2, s12, N, D; };
__device__ __forceinline__ SsimTerms ssim_terms(const float (&m)[5])
{
    SsimTerms q;
    // the reference's operations one by one (the build does not contract them): with size 1 the variances are exactly 0 as there
    q.s1 = m[2] - m[0] * m[0];
    q.s2 = m[3] - m[1] * m[1];
    q.s12 = m[4] - m[0] * m[1];
    q.N = q.s12 * q.s12 + SSIM_C3;
    q.D = q.s1 * q.s2 + SSIM_C3;
    return q;
}

// sum of v over the workgroup in a fixed order, valid in thread 0
__device__ __forceinline__ float block_sum_256(float v, float *red)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// grid (ceil(ow / 64), ceil(oh / 16), B).  map (may be NULL): [B,oh,ow]; partial (may be NULL): [B][gridDim.y][gridDim.x] tile sums
template <int K>
__global__ __launch_bounds__(256) void ssim_forward_kernel(const float *__restrict__ img1, const float *__restrict__ img2, int H, int W, int oh,
                                                           int ow, SsimWindow win, float *__restrict__ map, float *__restrict__ partial)
{
    __shared__ SsimSmem<K> sm;
    __shared__ float red[4];
    const int b = blockIdx.z, i0 = blockIdx.y * TH, j0 = blockIdx.x * TW;
    const size_t in_off = (size_t)b * H * W, out_off = (size_t)b * oh * ow;
    float m[ROWS][5];
    ssim_tile_moments<K>(img1 + in_off, img2 + in_off, H, W, i0, j0, win, sm, m);
    const int j = j0 + (threadIdx.x & 63), ib = i0 + (threadIdx.x >> 6) * ROWS;
    float sum = 0.f;
#pragma unroll
    for (int o = 0; o < ROWS; ++o) {
        const int i = ib + o;
        if (i < oh && j < ow) {
            const SsimTerms q = ssim_terms(m[o]);
            const float s = q.N / q.D;
            if (map) map[out_off + (size_t)i * ow + j] = s;
            sum += s;
        }
    }
    if (partial) {                                   // the same in every thread
        const float tot = block_sum_256(sum, red);
        if (threadIdx.x == 0) partial[((size_t)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = tot;
    }
}

// means[b] = (sum of the sample's n_tiles partial sums, in a fixed order) / count.  grid B
__global__ __launch_bounds__(256) void ssim_mean_kernel(const float *__restrict__ partial, int n_tiles, float count, float *__restrict__ means)
{
    __shared__ float red[4];
    const float *p = partial + (size_t)blockIdx.x * n_tiles;
    float v = 0.f;
    for (int i = threadIdx.x; i < n_tiles; i += 256) v += p[i];
    const float tot = block_sum_256(v, red);
    if (threadIdx.x == 0) means[blockIdx.x] = tot / count;
}

// The forward's grid.  fields: five planes of `plane` = B*oh*ow floats, g * ds/d{mu1, mu2, E[x^2], E[y^2], E[xy]} with
// g = dmap[b,i,j] (if given) + dmeans[b] / (oh*ow) (if given):
//   ds/ds12 = 2 s12 / D,  ds/ds1 = -N s2 / D^2,  ds/ds2 = -N s1 / D^2;  s1 = E[x^2] - mu1^2, s2 = E[y^2] - mu2^2, s12 = E[xy] - mu1 mu2
template <int K>
__global__ __launch_bounds__(256) void ssim_grad_fields_kernel(const float *__restrict__ img1, const float *__restrict__ img2, int H, int W,
                                                               int oh, int ow, SsimWindow win, const float *__restrict__ dmap,
                                                               const float *__restrict__ dmeans, float inv_count, float *__restrict__ fields,
                                                               size_t plane)
{
    __shared__ SsimSmem<K> sm;
    const int b = blockIdx.z, i0 = blockIdx.y * TH, j0 = blockIdx.x * TW;
    const size_t in_off = (size_t)b * H * W, out_off = (size_t)b * oh * ow;
    float m[ROWS][5];
    ssim_tile_moments<K>(img1 + in_off, img2 + in_off, H, W, i0, j0, win, sm, m);
    const int j = j0 + (threadIdx.x & 63), ib = i0 + (threadIdx.x >> 6) * ROWS;
    const float gmean = dmeans ? dmeans[b] * inv_count : 0.f;
#pragma unroll
    for (int o = 0; o < ROWS; ++o) {
        const int i = ib + o;
        if (i < oh && j < ow) {
            const size_t at = out_off + (size_t)i * ow + j;
            const float g = dmap ? dmap[at] + gmean : gmean;
            const SsimTerms q = ssim_terms(m[o]);
            const float invD = 1.0f / q.D;
            const float a = 2.0f * q.s12 * invD * g;             // g ds/ds12
            const float t = -q.N * invD * invD * g;
            const float b1 = t * q.s2, b2 = t * q.s1;            // g ds/ds1, g ds/ds2
            fields[at] = -(2.0f * m[o][0] * b1 + m[o][1] * a);
            fields[plane + at] = -(2.0f * m[o][1] * b2 + m[o][0] * a);
            fields[2 * plane + at] = b1;
            fields[3 * plane + at] = b2;
            fields[4 * plane + at] = a;
        }
    }
}

// grid (ceil(W / 64), ceil(H / 16), B): a tile of IMAGE pixels.  A(G)[i,j] = sum_{a,b} w[a] w[b] G[i-a, j-b] over the planes extended
// by zeros (the adjoint of the VALID correlation); d_img1 = A(g_mu1) + 2 x A(g_xx) + y A(g_xy), d_img2 likewise.  Either may be NULL.
template <int K>
__global__ __launch_bounds__(256) void ssim_adjoint_kernel(const float *__restrict__ fields, size_t plane, const float *__restrict__ img1,
                                                           const float *__restrict__ img2, int H, int W, int oh, int ow, SsimWindow win,
                                                           float *__restrict__ d_img1, float *__restrict__ d_img2)
{
    constexpr int RH = TH + K - 1, RW = TW + K - 1;
    __shared__ float raw[RH * RW];
    __shared__ float rp[5][RH * TW];
    const int t = threadIdx.x;
    const int b = blockIdx.z, i0 = blockIdx.y * TH, j0 = blockIdx.x * TW;
    const size_t in_off = (size_t)b * H * W, out_off = (size_t)b * oh * ow;
#pragma unroll 1
    for (int f = 0; f < 5; ++f) {
        const float *G = fields + (size_t)f * plane + out_off;
        for (int idx = t; idx < RH * RW; idx += 256) {
            const int r = idx / RW, c = idx - r * RW;
            const int gi = i0 - (K - 1) + r, gj = j0 - (K - 1) + c;
            raw[idx] = (gi >= 0 && gi < oh && gj >= 0 && gj < ow) ? G[gi * ow + gj] : 0.f;
        }
        __syncthreads();
        for (int idx = t; idx < RH * TW; idx += 256) {
            const int r = idx / TW, c = idx - r * TW;
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < K; ++k) acc = fmaf(win.w[k], raw[r * RW + c + (K - 1) - k], acc);
            rp[f][idx] = acc;
        }
        __syncthreads();
    }
    const int tx = t & 63, r0 = (t >> 6) * ROWS;
    float acc[ROWS][5];
#pragma unroll
    for (int o = 0; o < ROWS; ++o)
#pragma unroll
        for (int f = 0; f < 5; ++f) acc[o][f] = 0.f;
#pragma unroll
    for (int rr = 0; rr < ROWS + K - 1; ++rr) {
        float v[5];
#pragma unroll
        for (int f = 0; f < 5; ++f) v[f] = rp[f][(r0 + rr) * TW + tx];
#pragma unroll
        for (int o = 0; o < ROWS; ++o) {
            const int a = o + (K - 1) - rr;
            if (a >= 0 && a < K) {
#pragma unroll
                for (int f = 0; f < 5; ++f) acc[o][f] = fmaf(win.w[a], v[f], acc[o][f]);
            }
        }
    }
    const int j = j0 + tx;
#pragma unroll
    for (int o = 0; o < ROWS; ++o) {
        const int i = i0 + r0 + o;
        if (i < H && j < W) {
            const size_t at = in_off + (size_t)i * W + j;
            const float xv = img1[at], yv = img2[at];
            if (d_img1) d_img1[at] = acc[o][0] + 2.0f * xv * acc[o][2] + yv * acc[o][4];
            if (d_img2) d_img2[at] = acc[o][1] + 2.0f * yv * acc[o][3] + xv * acc[o][4];
        }
    }
}

// tf.nn.avg_pool(x, [1,2,2,1], [1,2,2,1], 'SAME') (utils.py:146-147): out [B, ceil(H/2), ceil(W/2), C]; a window over the edge
// averages the pixels that exist
__global__ __launch_bounds__(256) void avgpool2x2_same_kernel(const float *__restrict__ x, int H, int W, int C, int oh, int ow, long long total,
                                                              float *__restrict__ out)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int c = (int)(idx % C);
    long long p = idx / C;
    const int j = (int)(p % ow);
    p /= ow;
    const int i = (int)(p % oh);
    const long long b = p / oh;
    const bool r1 = 2 * i + 1 < H, c1 = 2 * j + 1 < W;
    const float *s = x + ((b * H + 2 * i) * W + 2 * j) * C + c;
    float top = s[0], bot = 0.f;
    if (c1) top += s[C];
    if (r1) {
        bot = s[(long long)W * C];
        if (c1) bot += s[(long long)W * C + C];
    }
    out[idx] = (top + bot) / (float)((r1 ? 2 : 1) * (c1 ? 2 : 1));
}

// its adjoint: dx[b,y,x,c] = dout[b, y/2, x/2, c] / (the number of pixels of that window)
__global__ __launch_bounds__(256) void avgpool2x2_same_backward_kernel(const float *__restrict__ dout, int H, int W, int C, int oh, int ow,
                                                                       long long total, float *__restrict__ dx)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int c = (int)(idx % C);
    long long p = idx / C;
    const int xw = (int)(p % W);
    p /= W;
    const int yh = (int)(p % H);
    const long long b = p / H;
    const int i = yh >> 1, j = xw >> 1;
    const int n = ((2 * i + 1 < H) ? 2 : 1) * ((2 * j + 1 < W) ? 2 : 1);
    dx[idx] = dout[((b * oh + i) * ow + j) * C + c] / (float)n;
}

inline dim3 tile_grid(int B, int h, int w) { return dim3((unsigned)((w + TW - 1) / TW), (unsigned)((h + TH - 1) / TH), (unsigned)B); }

}  // namespace

#define SSIM_FOR_SIZE(size, CALL)                                                                                                       \
    switch (size) {                                                                                                                     \
    case 1: CALL(1); break;                                                                                                             \
    case 2: CALL(2); break;                                                                                                             \
    case 3: CALL(3); break;                                                                                                             \
    case 4: CALL(4); break;                                                                                                             \
    case 5: CALL(5); break;                                                                                                             \
    case 6: CALL(6); break;                                                                                                             \
    case 7: CALL(7); break;                                                                                                             \
    case 8: CALL(8); break;                                                                                                             \
    case 9: CALL(9); break;                                                                                                             \
    case 10: CALL(10); break;                                                                                                           \
    case 11: CALL(11); break;                                                                                                           \
    default: return hipErrorInvalidValue;                                                                                               \
    }

size_t ssim_tiles_per_sample(int oh, int ow) { return (size_t)((oh + TH - 1) / TH) * (size_t)((ow + TW - 1) / TW); }

hipError_t launch_ssim_forward(const float *img1, const float *img2, int B, int H, int W, int size, const SsimWindow &win, float *map,
                               float *means, float *partial, hipStream_t stream)
{
    const int oh = H - size + 1, ow = W - size + 1;
    if (oh < 1 || ow < 1 || (means && !partial)) return hipErrorInvalidValue;
    const dim3 grid = tile_grid(B, oh, ow);
#define CALL(K) ssim_forward_kernel<K><<<grid, dim3(256), 0, stream>>>(img1, img2, H, W, oh, ow, win, map, means ? partial : nullptr)
    SSIM_FOR_SIZE(size, CALL)
#undef CALL
    if (means)
        ssim_mean_kernel<<<dim3((unsigned)B), dim3(256), 0, stream>>>(partial, (int)(grid.x * grid.y), (float)oh * (float)ow, means);
    return hipGetLastError();
}

hipError_t launch_ssim_backward(const float *img1, const float *img2, int B, int H, int W, int size, const SsimWindow &win, const float *dmap,
                                const float *dmeans, float *d_img1, float *d_img2, float *fields, hipStream_t stream)
{
    const int oh = H - size + 1, ow = W - size + 1;
    if (oh < 1 || ow < 1) return hipErrorInvalidValue;
    const size_t plane = (size_t)B * oh * ow;
    const float inv_count = 1.0f / ((float)oh * (float)ow);
    const dim3 fgrid = tile_grid(B, oh, ow), agrid = tile_grid(B, H, W);
#define CALL(K)                                                                                                                         \
    ssim_grad_fields_kernel<K><<<fgrid, dim3(256), 0, stream>>>(img1, img2, H, W, oh, ow, win, dmap, dmeans, inv_count, fields, plane); \
    ssim_adjoint_kernel<K><<<agrid, dim3(256), 0, stream>>>(fields, plane, img1, img2, H, W, oh, ow, win, d_img1, d_img2)
    SSIM_FOR_SIZE(size, CALL)
#undef CALL
    return hipGetLastError();
}

hipError_t launch_avgpool2x2_same(const float *x, int B, int H, int W, int C, float *out, hipStream_t stream)
{
    const int oh = (H + 1) / 2, ow = (W + 1) / 2;
    const long long total = (long long)B * oh * ow * C;
    avgpool2x2_same_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream>>>(x, H, W, C, oh, ow, total, out);
    return hipGetLastError();
}

hipError_t launch_avgpool2x2_same_backward(const float *dout, int B, int H, int W, int C, float *dx, hipStream_t stream)
{
    const int oh = (H + 1) / 2, ow = (W + 1) / 2;
    const long long total = (long long)B * H * W * C;
    avgpool2x2_same_backward_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream>>>(dout, H, W, C, oh, ow, total, dx);
    return hipGetLastError();
}

}  // namespace vstab
