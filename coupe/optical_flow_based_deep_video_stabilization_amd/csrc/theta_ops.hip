// HBM-side blocks of the theta regressors (reference model.py:152-184 Localizer, :375-455 dense_homo, :897-1024 flownetS_prehomo): TF
// SYMMETRIC padding, BatchNorm(moving statistics) + leaky relu of any slope alone and fused with the 2x2 SAME max pool, and the dense
// layers as a stream of W.  The convolutions between them run on conv_mfma.hip through vstab_conv_forward.  DESIGN.md section 23.
#include <hip/hip_runtime.h>

#include "theta_ops.h"

namespace vstab {

typedef float f32x4t __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------------------------ SYMMETRIC pad
// tf.pad "SYMMETRIC": the edge sample is repeated, index -1 reads 0 and index n reads n - 1.  p <= n keeps the result inside [0, n).
__device__ __forceinline__ int symmetric_index(int i, int n)
{
    return i < 0 ? -i - 1 : (i >= n ? 2 * n - 1 - i : i);
}

// One thread per channel quad of y.  VEC: C % 4 == 0 and x 16-byte aligned, the quad is one 16-byte load; otherwise up to four scalar
// loads.  Quads past C are zeros either way, and every store is 16 bytes.
template <bool VEC>
__global__ __launch_bounds__(256) void pad_symmetric_kernel(const float *__restrict__ x, int H, int W, int C, int p, float *__restrict__ y,
                                                            int Q, long long total)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int Ho = H + 2 * p, Wo = W + 2 * p;
    const int q = (int)(idx % Q);
    long long pix = idx / Q;
    const int j = (int)(pix % Wo);
    pix /= Wo;
    const int i = (int)(pix % Ho);
    const long long n = pix / Ho;
    const int si = symmetric_index(i - p, H), sj = symmetric_index(j - p, W);
    const float *src = x + ((n * H + si) * W + sj) * C + 4 * q;
    f32x4t v = {0.f, 0.f, 0.f, 0.f};
    if (VEC) {
        if (4 * q < C) v = *reinterpret_cast<const f32x4t *>(src);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (4 * q + e < C) v[e] = src[e];
    }
    reinterpret_cast<f32x4t *>(y)[idx] = v;
}

hipError_t launch_pad_symmetric(const float *x, int B, int H, int W, int C, int p, float *y, int cs_y, hipStream_t stream)
{
    const int Q = cs_y / 4;
    const long long total = (long long)B * (H + 2 * p) * (W + 2 * p) * Q;
    const dim3 grid((unsigned)((total + 255) / 256));
    if ((C & 3) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0)
        pad_symmetric_kernel<true><<<grid, dim3(256), 0, stream>>>(x, H, W, C, p, y, Q, total);
    else
        pad_symmetric_kernel<false><<<grid, dim3(256), 0, stream>>>(x, H, W, C, p, y, Q, total);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------- BatchNorm (moving statistics) + lrelu(slope)
__device__ __forceinline__ float lrelu_slope(float u, float slope)
{
    return u >= 0.f ? u : slope * u;
}

// the layer on one channel quad: m, s, b = moving mean, rstd, beta of the quad
__device__ __forceinline__ f32x4t bn_act_quad(f32x4t z, f32x4t m, f32x4t s, f32x4t b, float slope, int twice)
{
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float t = twice ? lrelu_slope(z[e], slope) : z[e];
        z[e] = lrelu_slope((t - m[e]) * s[e] + b[e], slope);
    }
    return z;
}

// rstd as bn_lrelu_inference_kernel (train_ops.hip) forms it
__device__ __forceinline__ f32x4t rstd_quad(const float *mov_var, int c, float eps)
{
    const f32x4t var = *reinterpret_cast<const f32x4t *>(mov_var + c);
    f32x4t s;
#pragma unroll
    for (int e = 0; e < 4; ++e) s[e] = (float)(1.0 / sqrt((double)var[e] + (double)eps));
    return s;
}

// In place, bn_lrelu_inference_kernel's shape: a thread keeps one channel quad for BN_ROWS rows, so the double divisions are paid once per
// 8 rows, and issues the rows' loads before it uses the first.
constexpr int BN_ROWS = 8;
__global__ __launch_bounds__(256) void bn_lrelu_slope_kernel(float *__restrict__ zy, int cs, int c_off, int C4, long long rows,
                                                             const float *__restrict__ mov_mean, const float *__restrict__ mov_var,
                                                             const float *__restrict__ beta, float eps, float slope, int twice)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long groups = (rows + BN_ROWS - 1) / BN_ROWS;
    if (idx >= groups * C4) return;
    const long long rg = idx / C4;
    const int c = (int)(idx - rg * C4) * 4;
    const f32x4t m = *reinterpret_cast<const f32x4t *>(mov_mean + c), b = *reinterpret_cast<const f32x4t *>(beta + c);
    const f32x4t s = rstd_quad(mov_var, c, eps);
    const long long r0 = rg * BN_ROWS;
    float *p = zy + r0 * cs + c_off + c;
    f32x4t v[BN_ROWS];
#pragma unroll
    for (int u = 0; u < BN_ROWS; ++u)
        if (r0 + u < rows) v[u] = *reinterpret_cast<const f32x4t *>(p + (long long)u * cs);
#pragma unroll
    for (int u = 0; u < BN_ROWS; ++u) {
        if (r0 + u >= rows) break;
        *reinterpret_cast<f32x4t *>(p + (long long)u * cs) = bn_act_quad(v[u], m, s, b, slope, twice);
    }
}

hipError_t launch_bn_lrelu_slope_inference(float *zy, long long rows, int cs, int c_off, int C, const float *beta, const float *mov_mean,
                                           const float *mov_var, float eps, float slope, int twice, hipStream_t stream)
{
    const long long n = (rows + BN_ROWS - 1) / BN_ROWS * (C / 4);
    bn_lrelu_slope_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream>>>(zy, cs, c_off, C / 4, rows, mov_mean, mov_var, beta, eps,
                                                                                      slope, twice);
    return hipGetLastError();
}

// The layer and MaxPool2d(2, 2, SAME) in one pass: a thread makes one channel quad of one pooled pixel from the up to four pixels of its
// window (the window is clipped where H or W is odd).  The activation is applied before the maximum, as the graph does.
__global__ __launch_bounds__(256) void bn_lrelu_slope_pool_kernel(const float *__restrict__ z, int H, int W, int C4, int Hp, int Wp,
                                                                  const float *__restrict__ mov_mean, const float *__restrict__ mov_var,
                                                                  const float *__restrict__ beta, float eps, float slope, int twice,
                                                                  float *__restrict__ out, long long total)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int q = (int)(idx % C4);
    long long pix = idx / C4;
    const int oj = (int)(pix % Wp);
    pix /= Wp;
    const int oi = (int)(pix % Hp);
    const long long n = pix / Hp;
    const f32x4t m = *reinterpret_cast<const f32x4t *>(mov_mean + 4 * q), b = *reinterpret_cast<const f32x4t *>(beta + 4 * q);
    const f32x4t s = rstd_quad(mov_var, 4 * q, eps);
    const f32x4t *src = reinterpret_cast<const f32x4t *>(z) + ((n * H + 2 * oi) * W + 2 * oj) * C4 + q;
    const bool right = 2 * oj + 1 < W, below = 2 * oi + 1 < H;
    f32x4t v[4];
    v[0] = src[0];
    v[1] = right ? src[C4] : v[0];
    v[2] = below ? src[(long long)W * C4] : v[0];
    v[3] = right && below ? src[(long long)W * C4 + C4] : v[0];
    f32x4t r = bn_act_quad(v[0], m, s, b, slope, twice);
#pragma unroll
    for (int t = 1; t < 4; ++t) {
        const f32x4t a = bn_act_quad(v[t], m, s, b, slope, twice);
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] = fmaxf(r[e], a[e]);
    }
    reinterpret_cast<f32x4t *>(out)[idx] = r;
}

hipError_t launch_bn_lrelu_slope_pool_inference(const float *z, int B, int H, int W, int C, const float *beta, const float *mov_mean,
                                                const float *mov_var, float eps, float slope, int twice, float *out, hipStream_t stream)
{
    const int Hp = (H + 1) / 2, Wp = (W + 1) / 2;
    const long long total = (long long)B * Hp * Wp * (C / 4);
    bn_lrelu_slope_pool_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream>>>(z, H, W, C / 4, Hp, Wp, mov_mean, mov_var, beta,
                                                                                               eps, slope, twice, out, total);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------------ dense
// y [B,N] = act(x [B,K] W [K,N] + b) with B <= 32: every output needs all of W, so the layer costs what reading W once costs, and the
// work is cut so that the whole device reads.  A wavefront owns DENSE_TILE_LANES * V columns and one slab of rows; each lane reads its
// V columns of a row (V = 4: 16 bytes, a wavefront covers 1 KiB of the row) and keeps B x V running sums, the rows of a slab taken in
// ascending order, four at a time.  x [b][k..k+3] is one 16-byte read at an address the whole wavefront shares.  The slab's sums go to
// partial [slab][B][N]; dense_combine_kernel adds the slabs in ascending order.  The cut depends on K and N alone.
constexpr int DENSE_TILE_LANES = 64;
constexpr int DENSE_WAVES = 1024;          // wavefronts asked for: four per CU of the 256, one per SIMD
constexpr int DENSE_MIN_GROUPS = 16;       // a slab is at least 64 rows, so that the partial sums stay small beside W
constexpr int DENSE_COMBINE_LANES = 16;    // dense_combine_kernel: slab ranges summed side by side, then added in order

DensePlan dense_plan(int K, int N)
{
    DensePlan d;
    d.vec = (N % 4 == 0) ? 4 : 1;
    d.tiles = (N + DENSE_TILE_LANES * d.vec - 1) / (DENSE_TILE_LANES * d.vec);
    const int groups = K / 4;
    const int target = DENSE_WAVES / d.tiles > 1 ? DENSE_WAVES / d.tiles : 1;
    int gps = (groups + target - 1) / target;
    if (gps < DENSE_MIN_GROUPS) gps = DENSE_MIN_GROUPS;
    d.rows = gps * 4;
    d.slabs = (K + d.rows - 1) / d.rows;
    return d;
}

template <int MB, int V>
__global__ __launch_bounds__(DENSE_TILE_LANES) void dense_slab_kernel(const float *__restrict__ x, int B, int K, int N,
                                                                      const float *__restrict__ W, int slab_rows, float *__restrict__ partial)
{
    const int col = ((int)blockIdx.x * DENSE_TILE_LANES + (int)threadIdx.x) * V;
    if (col >= N) return;                      // V = 4 only with N % 4 == 0: a live lane has all of its columns
    const int slab = blockIdx.y;
    const int k0 = slab * slab_rows;
    const int k1 = k0 + slab_rows < K ? k0 + slab_rows : K;
    float acc[MB][V];
#pragma unroll
    for (int b = 0; b < MB; ++b)
#pragma unroll
        for (int v = 0; v < V; ++v) acc[b][v] = 0.f;
    const float *wp = W + (long long)k0 * N + col;
#pragma unroll 4
    for (int k = k0; k < k1; k += 4, wp += 4LL * N) {
        float w[4][V];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (V == 4) {
                const f32x4t t = __builtin_nontemporal_load(reinterpret_cast<const f32x4t *>(wp + (long long)r * N));
#pragma unroll
                for (int v = 0; v < V; ++v) w[r][v] = t[v];
            } else {
                w[r][0] = __builtin_nontemporal_load(wp + (long long)r * N);
            }
        }
#pragma unroll
        for (int b = 0; b < MB; ++b) {
            const int row = b < B ? b : B - 1;         // rows past B repeat the last one and are not stored
            const f32x4t xv = *reinterpret_cast<const f32x4t *>(x + (long long)row * K + k);
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int v = 0; v < V; ++v) acc[b][v] = __builtin_fmaf(xv[r], w[r][v], acc[b][v]);
        }
    }
    float *dst = partial + (long long)slab * B * N + col;
#pragma unroll
    for (int b = 0; b < MB; ++b) {
        if (b >= B) break;
        if (V == 4) {
            const f32x4t t = {acc[b][0], acc[b][V > 1 ? 1 : 0], acc[b][V > 2 ? 2 : 0], acc[b][V > 3 ? 3 : 0]};
            *reinterpret_cast<f32x4t *>(dst + (long long)b * N) = t;
        } else {
            dst[(long long)b * N] = acc[b][0];
        }
    }
}

// y [o] = act(b + sum over the slabs of partial [slab][o]), o = row * N + column.  Sixteen lanes per output each add a contiguous range of
// slabs in ascending order, then lane 0 adds the sixteen sums in ascending order: the order is a function of the number of slabs alone.
__global__ __launch_bounds__(256) void dense_combine_kernel(const float *__restrict__ partial, int slabs, long long BN, int N,
                                                            const float *__restrict__ bias, int act, float slope,
                                                            const float *__restrict__ scale, const float *__restrict__ shift,
                                                            float *__restrict__ y)
{
    __shared__ float red[DENSE_COMBINE_LANES][17];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const long long o = (long long)blockIdx.x * 16 + tx;
    const int per = (slabs + DENSE_COMBINE_LANES - 1) / DENSE_COMBINE_LANES;
    float s = 0.f;
    if (o < BN) {
        const int s1 = (ty + 1) * per < slabs ? (ty + 1) * per : slabs;
        for (int i = ty * per; i < s1; ++i) s += partial[(long long)i * BN + o];
    }
    red[ty][tx] = s;
    __syncthreads();
    if (ty != 0 || o >= BN) return;
    float t = red[0][tx];
#pragma unroll
    for (int j = 1; j < DENSE_COMBINE_LANES; ++j) t += red[j][tx];
    const int n = (int)(o % N);
    float u = t + bias[n];
    if (act == 1) u = lrelu_slope(u, slope);
    else if (act == 2) u = tanhf(u);
    else if (act == 3) u = tanhf(u / 1000.f) * scale[n] + shift[n];
    y[o] = u;
}

template <int V>
static void launch_dense_slabs(const DensePlan &d, const float *x, int B, int K, int N, const float *W, float *partial, hipStream_t stream)
{
    const dim3 grid((unsigned)d.tiles, (unsigned)d.slabs), block(DENSE_TILE_LANES);
    if (B <= 1) dense_slab_kernel<1, V><<<grid, block, 0, stream>>>(x, B, K, N, W, d.rows, partial);
    else if (B <= 2) dense_slab_kernel<2, V><<<grid, block, 0, stream>>>(x, B, K, N, W, d.rows, partial);
    else if (B <= 4) dense_slab_kernel<4, V><<<grid, block, 0, stream>>>(x, B, K, N, W, d.rows, partial);
    else if (B <= 8) dense_slab_kernel<8, V><<<grid, block, 0, stream>>>(x, B, K, N, W, d.rows, partial);
    else if (B <= 16) dense_slab_kernel<16, V><<<grid, block, 0, stream>>>(x, B, K, N, W, d.rows, partial);
    else dense_slab_kernel<32, V><<<grid, block, 0, stream>>>(x, B, K, N, W, d.rows, partial);
}

hipError_t launch_dense_forward(const float *x, int B, int K, int N, const float *W, const float *b, int act, float slope, const float *scale,
                                const float *shift, float *y, float *partial, hipStream_t stream)
{
    const DensePlan d = dense_plan(K, N);
    if (d.vec == 4) launch_dense_slabs<4>(d, x, B, K, N, W, partial, stream);
    else launch_dense_slabs<1>(d, x, B, K, N, W, partial, stream);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const long long BN = (long long)B * N;
    dense_combine_kernel<<<dim3((unsigned)((BN + 15) / 16)), dim3(256), 0, stream>>>(partial, d.slabs, BN, N, b, act, slope, scale, shift, y);
    return hipGetLastError();
}

}  // namespace vstab
