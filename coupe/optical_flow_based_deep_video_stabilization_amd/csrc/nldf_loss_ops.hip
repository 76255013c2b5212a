// NLDF's training objective (NLDF.py:79-100 and :136-171): the contour term from the Sobel magnitude of the softmax and of the label,
// the IoU loss on it, the softmax cross-entropy, the accuracy, and the gradient of their sum with respect to Score.
//
//   P = softmax(Score)                                       both channels, the maximum subtracted
//   im_gradient(x)_c = sqrt(gx_c^2 + gy_c^2)                 gx, gy = 3x3 Sobel correlations of the clamp-to-edge extension of x_c
//   Prob_Grad  = tanh(im_gradient(P)_0 + im_gradient(P)_1)
//   label_Grad = im_gradient(label)_0 + im_gradient(label)_1 > contour_th ? 1 : 0
//   C_IoU_LOSS = 1 - 2 (I + 1) / (U + 1),  I = sum Prob_Grad label_Grad,  U = sum Prob_Grad^2 + sum label_Grad^2    (over the batch)
//   CE         = mean over pixels of -sum_c label_c log_softmax(Score)_c
//   Loss_Mean  = C_IoU_LOSS + CE,  accuracy = share of pixels with argmax Score == argmax label (a tie goes to channel 0)
//
// Forward: one workgroup per 32 x 8 tile keeps P and the label with a one-pixel halo in LDS (a halo cell holds the value at the CLAMPED
// coordinate, which is the SYMMETRIC pad of width one), every thread finishes one pixel, and the workgroup writes five partial sums in
// double.  nldf_loss_finish_kernel adds the partials in a fixed order: no atomics anywhere, two calls give the same bits.
//
// Backward (nldf_loss_backward_kernel, after the sums exist): a tile with a TWO-pixel halo of P and the label; over the one-pixel halo
// the adjoint coefficients  a_c = dLoss/dProb_Grad (1 - Prob_Grad^2) g_c / |g_c|  of gx_c and gy_c (0 where |g_c| == 0: the documented
// departure from TensorFlow's inf * 0); then every pixel GATHERS the adjoint of the clamped correlation from its 3x3 neighbours.  The
// Sobel filters are outer products of s = (1, 2, 1) and d = (-1, 0, 1) and the clamp acts per axis, so the weight with which output
// pixel q = p + e reaches input pixel p factors per axis into  w_k(p, e) = sum over taps t with clamp(q + t) == p of k[t]:  at a border the
// taps the clamp folded onto the edge pixel all land on it.  Then the softmax Jacobian, plus the cross-entropy term.
#include "vstab_internal.h"

namespace vstab {

namespace {

constexpr int TW = 32, TH = 8;                       // 256 threads, one pixel each: 32 pixels x 2 floats = one 256-byte row segment
constexpr int FW = TW + 2, FH = TH + 2;              // forward: one-pixel halo
constexpr int BW = TW + 4, BH = TH + 4;              // backward: two-pixel halo of P and label, one-pixel halo of the coefficients

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

__device__ __forceinline__ void softmax2(float s0, float s1, float &p0, float &p1)
{
    const float m = fmaxf(s0, s1);
    const float e0 = expf(s0 - m), e1 = expf(s1 - m);
    const float sum = e0 + e1;
    p0 = e0 / sum;
    p1 = e1 / sum;
}

// the two Sobel correlations at the centre (y, x) of a row-major LDS image with `pitch` floats per row
__device__ __forceinline__ void sobel_at(const float *im, int pitch, int y, int x, float &gx, float &gy)
{
    const float *r0 = im + (y - 1) * pitch + x, *r1 = r0 + pitch, *r2 = r1 + pitch;
    gx = ((r0[1] - r0[-1]) + 2.f * (r1[1] - r1[-1])) + (r2[1] - r2[-1]);
    gy = ((r2[-1] - r0[-1]) + 2.f * (r2[0] - r0[0])) + (r2[1] - r0[1]);
}

__device__ __forceinline__ float magnitude(float gx, float gy) { return sqrtf(gx * gx + gy * gy); }

// weight with which the output at q = p + e (e = -1, 0, 1) reaches the input at p along one axis of n pixels, for the 1-D factors
// s = (1, 2, 1) and d = (-1, 0, 1) of the Sobel filters; 0 for a q outside the image
__device__ __forceinline__ void axis_weights(int p, int n, float ws[3], float wd[3])
{
#pragma unroll
    for (int e = -1; e <= 1; ++e) {
        float s = 0.f, d = 0.f;
        const int q = p + e;
        if (q >= 0 && q < n) {
#pragma unroll
            for (int t = -1; t <= 1; ++t)
                if (clampi(q + t, n - 1) == p) {
                    s += t == 0 ? 2.f : 1.f;
                    d += (float)t;
                }
        }
        ws[e + 1] = s;
        wd[e + 1] = d;
    }
}

// sum of v over the 256 threads, in double and in a fixed order; every thread gets it.  red: 4 doubles; safe to call repeatedly
__device__ __forceinline__ double block_sum(double v, double *red)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    __syncthreads();                                  // the previous call's readers are done
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

struct TileId { int n, ty, tx; };
__device__ __forceinline__ TileId tile_of(unsigned block, int tiles_x, int tiles_y)
{
    TileId t;
    t.tx = (int)(block % (unsigned)tiles_x);
    const unsigned r = block / (unsigned)tiles_x;
    t.ty = (int)(r % (unsigned)tiles_y);
    t.n = (int)(r / (unsigned)tiles_y);
    return t;
}

__global__ __launch_bounds__(256) void nldf_loss_forward_kernel(const float *__restrict__ score, const float *__restrict__ label, int H, int W,
                                                                int tiles_x, int tiles_y, float contour_th, float *__restrict__ prob_grad,
                                                                float *__restrict__ label_grad, double *__restrict__ partial)
{
    __shared__ float sP[2][FH * FW], sL[2][FH * FW];
    __shared__ double red[4];
    const TileId t = tile_of(blockIdx.x, tiles_x, tiles_y);
    const int y0 = t.ty * TH, x0 = t.tx * TW;
    const long long base = (long long)t.n * H * W;
    for (int i = threadIdx.x; i < FH * FW; i += 256) {
        const int gy = clampi(y0 - 1 + i / FW, H - 1), gx = clampi(x0 - 1 + i % FW, W - 1);
        const long long px = base + (long long)gy * W + gx;
        const float2 s = *(const float2 *)(score + 2 * px), l = *(const float2 *)(label + 2 * px);
        softmax2(s.x, s.y, sP[0][i], sP[1][i]);
        sL[0][i] = l.x;
        sL[1][i] = l.y;
    }
    __syncthreads();
    const int ly = threadIdx.x / TW, lx = threadIdx.x % TW;
    const int y = y0 + ly, x = x0 + lx;
    double inter = 0.0, pp = 0.0, gg = 0.0, ce = 0.0, hit = 0.0;
    if (y < H && x < W) {
        float gx, gy;
        sobel_at(sP[0], FW, ly + 1, lx + 1, gx, gy);
        float sp = magnitude(gx, gy);
        sobel_at(sP[1], FW, ly + 1, lx + 1, gx, gy);
        sp += magnitude(gx, gy);
        sobel_at(sL[0], FW, ly + 1, lx + 1, gx, gy);
        float sl = magnitude(gx, gy);
        sobel_at(sL[1], FW, ly + 1, lx + 1, gx, gy);
        sl += magnitude(gx, gy);
        const float pred = tanhf(sp), gt = sl > contour_th ? 1.f : 0.f;
        const long long px = base + (long long)y * W + x;
        if (prob_grad) prob_grad[px] = pred;
        if (label_grad) label_grad[px] = gt;
        const float2 s = *(const float2 *)(score + 2 * px);
        const float l0 = sL[0][(ly + 1) * FW + lx + 1], l1 = sL[1][(ly + 1) * FW + lx + 1];
        const float m = fmaxf(s.x, s.y);
        const float lse = m + logf(expf(s.x - m) + expf(s.y - m));
        ce = (double)(-(l0 * (s.x - lse) + l1 * (s.y - lse)));
        inter = (double)(pred * gt);
        pp = (double)(pred * pred);
        gg = (double)gt;                                          // gt^2 == gt
        hit = ((s.y > s.x) == (l1 > l0)) ? 1.0 : 0.0;             // argmax with ties to channel 0
    }
    inter = block_sum(inter, red);
    pp = block_sum(pp, red);
    gg = block_sum(gg, red);
    ce = block_sum(ce, red);
    hit = block_sum(hit, red);
    if (threadIdx.x == 0) {
        double *o = partial + 5 * (size_t)blockIdx.x;
        o[0] = inter; o[1] = pp; o[2] = gg; o[3] = ce; o[4] = hit;
    }
}

// one workgroup: thread t adds partials t, t + 256, ... in that order, then the 256 sums are added as a fixed tree.
// sums[0..1] = I, U for the backward; scalars = Loss_Mean, C_IoU_LOSS, CE, accuracy
__global__ __launch_bounds__(256) void nldf_loss_finish_kernel(const double *__restrict__ partial, unsigned nblocks, double npix,
                                                               double *__restrict__ sums, float *__restrict__ scalars)
{
    __shared__ double red[4];
    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (unsigned b = threadIdx.x; b < nblocks; b += 256)
#pragma unroll
        for (int k = 0; k < 5; ++k) v[k] += partial[5 * (size_t)b + k];
#pragma unroll
    for (int k = 0; k < 5; ++k) v[k] = block_sum(v[k], red);
    if (threadIdx.x == 0) {
        const double I = v[0], U = v[1] + v[2];
        const double iou = 1.0 - 2.0 * (I + 1.0) / (U + 1.0), ce = v[3] / npix;
        sums[0] = I;
        sums[1] = U;
        scalars[0] = (float)(iou + ce);
        scalars[1] = (float)iou;
        scalars[2] = (float)ce;
        scalars[3] = (float)(v[4] / npix);
    }
}

__global__ __launch_bounds__(256) void nldf_loss_backward_kernel(const float *__restrict__ score, const float *__restrict__ label, int H, int W,
                                                                 int tiles_x, int tiles_y, float contour_th, const double *__restrict__ sums,
                                                                 float inv_npix, float dscale, float *__restrict__ dscore)
{
    __shared__ float sP[2][BH * BW], sL[2][BH * BW];
    __shared__ float sA[4][FH * FW];                  // ax0, ay0, ax1, ay1 over the one-pixel halo
    const TileId t = tile_of(blockIdx.x, tiles_x, tiles_y);
    const int y0 = t.ty * TH, x0 = t.tx * TW;
    const long long base = (long long)t.n * H * W;
    for (int i = threadIdx.x; i < BH * BW; i += 256) {
        const int gy = clampi(y0 - 2 + i / BW, H - 1), gx = clampi(x0 - 2 + i % BW, W - 1);
        const long long px = base + (long long)gy * W + gx;
        const float2 s = *(const float2 *)(score + 2 * px), l = *(const float2 *)(label + 2 * px);
        softmax2(s.x, s.y, sP[0][i], sP[1][i]);
        sL[0][i] = l.x;
        sL[1][i] = l.y;
    }
    // d C_IoU_LOSS / d pred = c_gt gt + c_pred pred
    const double I = sums[0], U = sums[1];
    const float c_gt = (float)(-2.0 / (U + 1.0)), c_pred = (float)(4.0 * (I + 1.0) / ((U + 1.0) * (U + 1.0)));
    __syncthreads();
    for (int i = threadIdx.x; i < FH * FW; i += 256) {
        const int cy = i / FW, cx = i % FW;                       // cell of the one-pixel halo; (cy + 1, cx + 1) in the two-pixel one
        const int qy = y0 - 1 + cy, qx = x0 - 1 + cx;
        float a[4] = {0.f, 0.f, 0.f, 0.f};
        if (qy >= 0 && qy < H && qx >= 0 && qx < W) {
            float gx[2], gy[2], mag[2], gl0x, gl0y, gl1x, gl1y;
            sobel_at(sP[0], BW, cy + 1, cx + 1, gx[0], gy[0]);
            sobel_at(sP[1], BW, cy + 1, cx + 1, gx[1], gy[1]);
            sobel_at(sL[0], BW, cy + 1, cx + 1, gl0x, gl0y);
            sobel_at(sL[1], BW, cy + 1, cx + 1, gl1x, gl1y);
            mag[0] = magnitude(gx[0], gy[0]);
            mag[1] = magnitude(gx[1], gy[1]);
            const float pred = tanhf(mag[0] + mag[1]);
            const float gt = magnitude(gl0x, gl0y) + magnitude(gl1x, gl1y) > contour_th ? 1.f : 0.f;
            const float coef = (c_gt * gt + c_pred * pred) * (1.f - pred * pred);
#pragma unroll
            for (int c = 0; c < 2; ++c)
                if (mag[c] > 0.f) {
                    a[2 * c] = coef * (gx[c] / mag[c]);
                    a[2 * c + 1] = coef * (gy[c] / mag[c]);
                }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) sA[k][i] = a[k];
    }
    __syncthreads();
    const int ly = threadIdx.x / TW, lx = threadIdx.x % TW;
    const int y = y0 + ly, x = x0 + lx;
    if (y >= H || x >= W) return;
    float sy[3], dy[3], sx[3], dx[3];
    axis_weights(y, H, sy, dy);
    axis_weights(x, W, sx, dx);
    float dP[2] = {0.f, 0.f};
#pragma unroll
    for (int ey = 0; ey < 3; ++ey)
#pragma unroll
        for (int ex = 0; ex < 3; ++ex) {
            const int i = (ly + ey) * FW + lx + ex;               // q = p + (ey - 1, ex - 1) in the one-pixel halo
            const float wx = sy[ey] * dx[ex], wy = dy[ey] * sx[ex];    // fx = s (rows) x d (columns), fy = d x s
            dP[0] += wx * sA[0][i] + wy * sA[1][i];
            dP[1] += wx * sA[2][i] + wy * sA[3][i];
        }
    const int c = (ly + 2) * BW + lx + 2;
    const float p0 = sP[0][c], p1 = sP[1][c], l0 = sL[0][c], l1 = sL[1][c];
    const float dot = p0 * dP[0] + p1 * dP[1], lsum = l0 + l1;
    float2 out;
    out.x = dscale * (p0 * (dP[0] - dot) + (p0 * lsum - l0) * inv_npix);
    out.y = dscale * (p1 * (dP[1] - dot) + (p1 * lsum - l1) * inv_npix);
    *(float2 *)(dscore + 2 * (base + (long long)y * W + x)) = out;
}

// ---- im_gradient by itself, [B,H,W,C] with any small C: one thread per element, neighbours read at clamped coordinates
__device__ __forceinline__ void sobel_global(const float *__restrict__ img, int H, int W, int C, int y, int x, float &gx, float &gy)
{
    const int ym = clampi(y - 1, H - 1), yp = clampi(y + 1, H - 1), xm = clampi(x - 1, W - 1), xp = clampi(x + 1, W - 1);
    const float *r0 = img + (long long)ym * W * C, *r1 = img + (long long)y * W * C, *r2 = img + (long long)yp * W * C;
    const int a = xm * C, b = x * C, c = xp * C;
    gx = ((r0[c] - r0[a]) + 2.f * (r1[c] - r1[a])) + (r2[c] - r2[a]);
    gy = ((r2[a] - r0[a]) + 2.f * (r2[b] - r0[b])) + (r2[c] - r0[c]);
}

__global__ __launch_bounds__(256) void sobel_magnitude_kernel(const float *__restrict__ x, int H, int W, int C, long long total,
                                                              float *__restrict__ out)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int c = (int)(idx % C);
    const long long px = idx / C;
    const int xx = (int)(px % W), yy = (int)((px / W) % H);
    const long long n = px / ((long long)W * H);
    float gx, gy;
    sobel_global(x + n * H * W * C + c, H, W, C, yy, xx, gx, gy);
    out[idx] = magnitude(gx, gy);
}

__global__ __launch_bounds__(256) void sobel_magnitude_backward_kernel(const float *__restrict__ x, const float *__restrict__ dout, int H, int W,
                                                                       int C, long long total, float *__restrict__ dxo)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int c = (int)(idx % C);
    const long long px = idx / C;
    const int xx = (int)(px % W), yy = (int)((px / W) % H);
    const long long n = px / ((long long)W * H);
    const float *img = x + n * H * W * C + c, *dimg = dout + n * H * W * C + c;
    float sy[3], dy[3], sx[3], dx[3];
    axis_weights(yy, H, sy, dy);
    axis_weights(xx, W, sx, dx);
    float acc = 0.f;
#pragma unroll
    for (int ey = 0; ey < 3; ++ey)
#pragma unroll
        for (int ex = 0; ex < 3; ++ex) {
            const int qy = yy + ey - 1, qx = xx + ex - 1;
            if (qy < 0 || qy >= H || qx < 0 || qx >= W) continue;
            float gx, gy;
            sobel_global(img, H, W, C, qy, qx, gx, gy);
            const float mag = magnitude(gx, gy);
            if (mag > 0.f) {
                const float g = dimg[((long long)qy * W + qx) * C];
                acc += (sy[ey] * dx[ex]) * (g * (gx / mag)) + (dy[ey] * sx[ex]) * (g * (gy / mag));
            }
        }
    dxo[idx] = acc;
}

// ---- the reductions behind Loss_IoU, Loss_Contour and L2.  partial: 3 doubles per workgroup
__global__ __launch_bounds__(256) void nldf_reduce_partial_kernel(int mode, const float *__restrict__ a, const float *__restrict__ b, long long n,
                                                                  double *__restrict__ partial)
{
    __shared__ double red[4];
    double v0 = 0.0, v1 = 0.0, v2 = 0.0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float p = a[i];
        if (mode == NLDF_REDUCE_IOU) {
            const float g = b[i];
            v0 += (double)(p * g);
            v1 += (double)(p * p);
            v2 += (double)(g * g);
        } else if (mode == NLDF_REDUCE_CONTOUR) {
            const float g = b[i];
            v0 += (double)(-g * logf(p + 1e-5f) - (1.f - g) * logf(1.f - p + 1e-5f));
        } else {
            v0 += (double)(p * p);
        }
    }
    v0 = block_sum(v0, red);
    v1 = block_sum(v1, red);
    v2 = block_sum(v2, red);
    if (threadIdx.x == 0) {
        double *o = partial + 3 * (size_t)blockIdx.x;
        o[0] = v0; o[1] = v1; o[2] = v2;
    }
}

__global__ __launch_bounds__(256) void nldf_reduce_finish_kernel(int mode, const double *__restrict__ partial, unsigned nblocks, double n, float wd,
                                                                 double *__restrict__ sums, float *__restrict__ value)
{
    __shared__ double red[4];
    double v[3] = {0.0, 0.0, 0.0};
    for (unsigned blk = threadIdx.x; blk < nblocks; blk += 256)
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] += partial[3 * (size_t)blk + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = block_sum(v[k], red);
    if (threadIdx.x == 0) {
        sums[0] = v[0];
        sums[1] = v[1] + v[2];
        if (mode == NLDF_REDUCE_IOU) *value = (float)(1.0 - 2.0 * (v[0] + 1.0) / (v[1] + v[2] + 1.0));
        else if (mode == NLDF_REDUCE_CONTOUR) *value = (float)(v[0] / n);
        else *value = (float)((double)wd * v[0] / 2.0);
    }
}

__global__ __launch_bounds__(256) void nldf_reduce_grad_kernel(int mode, const float *__restrict__ a, const float *__restrict__ b, long long n,
                                                               float wd, const double *__restrict__ sums, float *__restrict__ grad)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float p = a[i];
    if (mode == NLDF_REDUCE_IOU) {
        const double I = sums[0], U = sums[1];
        const float c_gt = (float)(-2.0 / (U + 1.0)), c_pred = (float)(4.0 * (I + 1.0) / ((U + 1.0) * (U + 1.0)));
        grad[i] = c_gt * b[i] + c_pred * p;
    } else if (mode == NLDF_REDUCE_CONTOUR) {
        const float g = b[i];
        grad[i] = (-g / (p + 1e-5f) + (1.f - g) / (1.f - p + 1e-5f)) / (float)n;
    } else {
        grad[i] = wd * p;
    }
}

}  // namespace

size_t nldf_loss_tiles(int B, int H, int W) { return (size_t)B * (size_t)((H + TH - 1) / TH) * (size_t)((W + TW - 1) / TW); }

hipError_t launch_nldf_loss(const float *score, const float *label, int B, int H, int W, float contour_th, float *scalars, float *prob_grad,
                            float *label_grad, float *dscore, float dscale, double *workspace, hipStream_t stream)
{
    const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH;
    const size_t nblocks = nldf_loss_tiles(B, H, W);
    if (nblocks == 0 || nblocks >= (1ull << 31)) return hipErrorInvalidValue;
    double *sums = workspace, *partial = workspace + 2;
    const double npix = (double)B * H * W;
    nldf_loss_forward_kernel<<<dim3((unsigned)nblocks), dim3(256), 0, stream>>>(score, label, H, W, tiles_x, tiles_y, contour_th, prob_grad,
                                                                                label_grad, partial);
    nldf_loss_finish_kernel<<<dim3(1), dim3(256), 0, stream>>>(partial, (unsigned)nblocks, npix, sums, scalars);
    if (dscore)
        nldf_loss_backward_kernel<<<dim3((unsigned)nblocks), dim3(256), 0, stream>>>(score, label, H, W, tiles_x, tiles_y, contour_th, sums,
                                                                                     (float)(1.0 / npix), dscale, dscore);
    return hipGetLastError();
}

hipError_t launch_sobel_magnitude(const float *x, int B, int H, int W, int C, float *out, hipStream_t stream)
{
    const long long total = (long long)B * H * W * C;
    sobel_magnitude_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream>>>(x, H, W, C, total, out);
    return hipGetLastError();
}

hipError_t launch_sobel_magnitude_backward(const float *x, const float *dout, int B, int H, int W, int C, float *dx, hipStream_t stream)
{
    const long long total = (long long)B * H * W * C;
    sobel_magnitude_backward_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream>>>(x, dout, H, W, C, total, dx);
    return hipGetLastError();
}

unsigned nldf_reduce_blocks(long long n) { return (unsigned)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024); }

hipError_t launch_nldf_reduce(int mode, const float *a, const float *b, long long n, float wd, float *value, float *grad, double *workspace,
                              hipStream_t stream)
{
    const unsigned nblocks = nldf_reduce_blocks(n);
    if (nblocks == 0) return hipErrorInvalidValue;
    double *sums = workspace, *partial = workspace + 2;
    nldf_reduce_partial_kernel<<<dim3(nblocks), dim3(256), 0, stream>>>(mode, a, b, n, partial);
    nldf_reduce_finish_kernel<<<dim3(1), dim3(256), 0, stream>>>(mode, partial, nblocks, (double)n, wd, sums, value);
    if (grad)
        nldf_reduce_grad_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream>>>(mode, a, b, n, wd, sums, grad);
    return hipGetLastError();
}

}  // namespace vstab
