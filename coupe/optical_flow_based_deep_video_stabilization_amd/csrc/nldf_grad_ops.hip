// Backward pieces of the NLDF saliency head that the training convolutions do not cover: the Score stage
// (softmax share, the per-sample pixel sums that are Global_Score's gradient, the 640 -> 2 Local_Score layer both ways, the tiny
// Global_Score layer), the contrast layer's adjoint fused with Fea_Pk's ReLU gate, and the gate of an Up slice.  All are
// bandwidth-bound passes: float4 on the channel axis, reductions by wave shuffle, then LDS, then a second launch that adds the
// slabs in a fixed order.  No float atomics: two runs give the same bits.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "vstab_internal.h"

namespace vstab {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// ---- Score = Local_Score + Global_Score, Prob = softmax(Score)[..., 0].  The gradient at Score is dscore plus Prob's share,
// t = p0 (1 - p0) dprob on channel 0 and -t on channel 1; it is Local_Score's gradient as it stands (written to dls only when
// there is a dprob: otherwise dscore itself serves) and its sum over a sample's pixels is Global_Score's.  grid (SCORE_SLABS, B):
// slab s of sample n sums a contiguous run of pixels into part[(n * SCORE_SLABS + s) * 2 + c].
constexpr int SCORE_SLABS = 64;

__global__ __launch_bounds__(256) void nldf_score_grad_kernel(const float2 *__restrict__ dscore, const float *__restrict__ prob,
                                                              const float *__restrict__ dprob, int npix, float2 *__restrict__ dls,
                                                              float *__restrict__ part)
{
    __shared__ float red[4][2];
    const int n = blockIdx.y, s = blockIdx.x;
    const int per = (npix + SCORE_SLABS - 1) / SCORE_SLABS;
    const int p0 = s * per, p1 = min(p0 + per, npix);
    const long long base = (long long)n * npix;
    float a0 = 0.f, a1 = 0.f;
    for (int p = p0 + threadIdx.x; p < p1; p += 256) {
        float2 d = dscore[base + p];
        if (dprob) {
            const float q = prob[base + p];
            const float t = q * (1.f - q) * dprob[base + p];
            d.x += t; d.y -= t;
            dls[base + p] = d;
        }
        a0 += d.x; a1 += d.y;
    }
    a0 = wave_sum(a0); a1 = wave_sum(a1);
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = a0; red[threadIdx.x >> 6][1] = a1; }
    __syncthreads();
    if (threadIdx.x < 2) {
        const int c = threadIdx.x;
        part[((long long)n * SCORE_SLABS + s) * 2 + c] = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
    }
}

// One workgroup: dgs [B][2] = the slabs added in order; both score biases' gradient = sum_b dgs; Global_Score (1x1, 128 -> 2 on the
// B rows of Fea_Global): dW_gs [128][2] = sum_b fg[b,:]^T dgs[b,:], dfg [B][128] = dgs[b,0] W[:,0] + dgs[b,1] W[:,1] (+ dfea_global).
// fg == NULL: the sums and the biases only.  B <= 64.
__global__ __launch_bounds__(256) void nldf_score_fold_kernel(const float *__restrict__ part, int B, const float *__restrict__ fg,
                                                              const float *__restrict__ Wgs, const float *__restrict__ dfea_global,
                                                              float *__restrict__ dgs, float *__restrict__ dfg, float *__restrict__ dW_gs,
                                                              float *__restrict__ db_gs, float *__restrict__ db_ls, int accumulate)
{
    __shared__ float sg[128];
    const int t = threadIdx.x;
    if (t < 2 * B) {
        const int n = t >> 1, c = t & 1;
        float s = 0.f;
        for (int k = 0; k < SCORE_SLABS; ++k) s += part[((long long)n * SCORE_SLABS + k) * 2 + c];
        sg[t] = s;
        dgs[t] = s;
    }
    __syncthreads();
    if (t < 2) {
        float s = 0.f;
        for (int n = 0; n < B; ++n) s += sg[2 * n + t];
        if (db_gs) db_gs[t] = accumulate ? db_gs[t] + s : s;
        if (db_ls) db_ls[t] = accumulate ? db_ls[t] + s : s;
    }
    if (!fg) return;
    if (dW_gs) {
        const int c = t >> 1, o = t & 1;               // 256 threads = 128 x 2
        float s = 0.f;
        for (int n = 0; n < B; ++n) s += fg[n * 128 + c] * sg[2 * n + o];
        dW_gs[t] = accumulate ? dW_gs[t] + s : s;
    }
    if (dfg)
        for (int i = t; i < B * 128; i += 256) {
            const int n = i >> 7, c = i & 127;
            float r = sg[2 * n] * Wgs[2 * c] + sg[2 * n + 1] * Wgs[2 * c + 1];
            if (dfea_global) r += dfea_global[i];
            dfg[i] = r;
        }
}

hipError_t launch_nldf_score_grad(const float *dscore, const float *prob, const float *dprob, int B, int npix, float *dls, float *part,
                                  hipStream_t stream)
{
    if (B < 1 || B > 64 || npix < 1 || (dprob && (!prob || !dls))) return hipErrorInvalidValue;
    nldf_score_grad_kernel<<<dim3(SCORE_SLABS, (unsigned)B), dim3(256), 0, stream>>>(reinterpret_cast<const float2 *>(dscore), prob, dprob, npix,
                                                                                     reinterpret_cast<float2 *>(dls), part);
    return hipGetLastError();
}

size_t nldf_score_part_floats(int B) { return (size_t)B * SCORE_SLABS * 2; }

hipError_t launch_nldf_score_fold(const float *part, int B, const float *fg, const float *Wgs, const float *dfea_global, float *dgs, float *dfg,
                                  float *dW_gs, float *db_gs, float *db_ls, int accumulate, hipStream_t stream)
{
    if (B < 1 || B > 64 || !dgs || (fg && !Wgs)) return hipErrorInvalidValue;
    nldf_score_fold_kernel<<<dim3(1), dim3(256), 0, stream>>>(part, B, fg, Wgs, dfea_global, dgs, dfg, dW_gs, db_gs, db_ls, accumulate ? 1 : 0);
    return hipGetLastError();
}

// ---- Local_Score (1x1, C -> 2; C % 4 == 0, C <= 1024) is too narrow for the GEMM launchers (2 columns).  Its input gradient:
// dlf[p,:] = dls[p,0] W[:,0] + dls[p,1] W[:,1] (+ dlocal_fea[p,:]), one float4 per thread, W [C][2] de-interleaved in LDS.
__global__ __launch_bounds__(256) void local_score_dgrad_kernel(const float2 *__restrict__ dls, const float *__restrict__ W, int C4,
                                                                const f32x4 *__restrict__ dlocal_fea, long long total, f32x4 *__restrict__ dlf)
{
    __shared__ float w0[1024], w1[1024];
    for (int i = threadIdx.x; i < C4 * 4; i += 256) { w0[i] = W[2 * i]; w1[i] = W[2 * i + 1]; }
    __syncthreads();
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
        const long long pix = i / C4;
        const int q = (int)(i - pix * C4);
        const float2 d = dls[pix];
        f32x4 r;
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] = d.x * w0[4 * q + e] + d.y * w1[4 * q + e];
        if (dlocal_fea) r += dlocal_fea[i];
        dlf[i] = r;
    }
}

hipError_t launch_local_score_dgrad(const float *dls, const float *W, long long npix, int C, const float *dlocal_fea, float *dlf, hipStream_t stream)
{
    if (npix < 1 || C < 4 || (C & 3) || C > 1024) return hipErrorInvalidValue;
    const long long total = npix * (C / 4);
    const long long blocks = std::min<long long>((total + 255) / 256, 256 * 16);
    local_score_dgrad_kernel<<<dim3((unsigned)blocks), dim3(256), 0, stream>>>(reinterpret_cast<const float2 *>(dls), W, C / 4,
                                                                               reinterpret_cast<const f32x4 *>(dlocal_fea), total,
                                                                               reinterpret_cast<f32x4 *>(dlf));
    return hipGetLastError();
}

// Its filter gradient dW [C][2] = sum_p lf[p,:]^T dls[p,:]: a workgroup is 2 pixel lanes x C/4 float4 lanes (C = 640: 320 threads, five
// waves), each thread sums its float4 of channels against both score channels over a strided share of the pixels; the two pixel lanes
// fold through LDS and the workgroup writes one [C][2] slab.  The second launch adds the slabs in order.
constexpr int LS_WGRAD_SLABS = 512;

__global__ __launch_bounds__(512) void local_score_wgrad_kernel(const f32x4 *__restrict__ lf, const float2 *__restrict__ dls, long long npix, int C4,
                                                                float *__restrict__ slabs)
{
    extern __shared__ f32x4 sm[];                      // [2][C4]: pixel lane 1's sums
    const int q = threadIdx.x % C4, pl = threadIdx.x / C4;
    f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
    for (long long p = (long long)blockIdx.x * 2 + pl; p < npix; p += (long long)gridDim.x * 2) {
        const f32x4 v = lf[p * C4 + q];
        const float2 d = dls[p];
        a0 += v * d.x; a1 += v * d.y;
    }
    if (pl == 1) { sm[q] = a0; sm[C4 + q] = a1; }
    __syncthreads();
    if (pl == 0) {
        a0 += sm[q]; a1 += sm[C4 + q];
        float *o = slabs + (long long)blockIdx.x * C4 * 8 + q * 8;
        *reinterpret_cast<f32x4 *>(o) = f32x4{a0[0], a1[0], a0[1], a1[1]};
        *reinterpret_cast<f32x4 *>(o + 4) = f32x4{a0[2], a1[2], a0[3], a1[3]};
    }
}

__global__ __launch_bounds__(256) void slab_fold_kernel(const float *__restrict__ slabs, int nslabs, int n, float *__restrict__ out, int accumulate)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    // 16 interleaved chains, then a tree: the order is fixed, and no chain is longer than nslabs / 16 additions
    float a[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) a[j] = 0.f;
    for (int k = 0; k < nslabs; k += 16)
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (k + j < nslabs) a[j] += slabs[(long long)(k + j) * n + i];
#pragma unroll
    for (int w = 8; w >= 1; w >>= 1)
#pragma unroll
        for (int j = 0; j < w; ++j) a[j] += a[j + w];
    out[i] = accumulate ? out[i] + a[0] : a[0];
}

size_t local_score_wgrad_scratch_floats(int C) { return (size_t)LS_WGRAD_SLABS * C * 2; }

hipError_t launch_local_score_wgrad(const float *lf, const float *dls, long long npix, int C, float *dW, int accumulate, float *scratch,
                                    hipStream_t stream)
{
    if (npix < 1 || C < 4 || (C & 3) || C > 1024) return hipErrorInvalidValue;
    const int C4 = C / 4;
    local_score_wgrad_kernel<<<dim3(LS_WGRAD_SLABS), dim3(2 * C4), 2 * C4 * sizeof(f32x4), stream>>>(reinterpret_cast<const f32x4 *>(lf),
                                                                                                     reinterpret_cast<const float2 *>(dls), npix, C4, scratch);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    slab_fold_kernel<<<dim3((2 * C + 255) / 256), dim3(256), 0, stream>>>(scratch, LS_WGRAD_SLABS, 2 * C, dW, accumulate ? 1 : 0);
    return hipGetLastError();
}

// ---- Contrast_Layer (x - avg3x3 of the one-pixel SYMMETRIC pad of x) is its own adjoint: the 1-D clamped box sum is a symmetric
// matrix (row 0 is [2,1,0,...], row 1 [1,1,1,0,...], a single row [3]).  With cat = [P | LC | ...] and dcat = [dP | dLC | ...] (Cs-wide
// pixels, C channels each), Fea_Pk's pre-activation gradient is (P > 0) ? dP + dLC - avg3x3_sym(dLC) : 0, written over dP.  The
// neighbourhood is read from the dLC slice, the write goes to the dP slice: no thread reads what another writes.
__global__ __launch_bounds__(256) void contrast_gate_backward_kernel(const float *__restrict__ act, float *__restrict__ dcat, int B, int H, int W, int C4,
                                                                     int Cs)
{
    const long long total = (long long)B * H * W * C4;
    const long long stride = (long long)gridDim.x * 256;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += stride) {
        const int c = (int)(idx % C4);
        const long long pix = idx / C4;
        const int n = (int)(pix / (H * W));
        const int rem = (int)(pix - (long long)n * H * W);
        const int y = rem / W, x = rem - y * W;
        const float *b = dcat + (long long)n * H * W * Cs + C4 * 4 + c * 4;          // the dLC slice of this sample
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
            const int yy = min(max(y + dy, 0), H - 1);
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const int xx = min(max(x + dx, 0), W - 1);
                s += *reinterpret_cast<const f32x4 *>(b + ((long long)yy * W + xx) * Cs);
            }
        }
        const f32x4 ctr = *reinterpret_cast<const f32x4 *>(b + ((long long)y * W + x) * Cs);
        float *dp = dcat + pix * Cs + c * 4;
        const f32x4 g = *reinterpret_cast<const f32x4 *>(dp);
        const f32x4 a = *reinterpret_cast<const f32x4 *>(act + pix * Cs + c * 4);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = a[e] > 0.f ? (g[e] + ctr[e]) - s[e] / 9.0f : 0.f;
        *reinterpret_cast<f32x4 *>(dp) = o;
    }
}

hipError_t launch_contrast_gate_backward(const float *act, float *dcat, int B, int H, int W, int C, int Cs, hipStream_t stream)
{
    if (B < 1 || H < 1 || W < 1 || C < 4 || (C & 3) || (Cs & 3) || Cs < 2 * C) return hipErrorInvalidValue;
    const long long total = (long long)B * H * W * (C / 4);
    const long long blocks = std::min<long long>((total + 255) / 256, 256 * 16);        // grid-stride above 16 workgroups per CU
    contrast_gate_backward_kernel<<<dim3((unsigned)blocks), dim3(256), 0, stream>>>(act, dcat, B, H, W, C / 4, Cs);
    return hipGetLastError();
}

// ---- ReLU gate of a channel slice in place: d[row, c_off + c] = act[row, c_off + c] > 0 ? d : 0 for c < C (the Up slice of a concat
// buffer; its bias gradient is launch_column_sum over the gated slice).
__global__ __launch_bounds__(256) void slice_gate_kernel(const float *__restrict__ act, float *__restrict__ d, long long rows, int Cs, int c_off, int C4)
{
    const long long total = rows * C4;
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
        const long long r = i / C4;
        const long long off = r * Cs + c_off + (i - r * C4) * 4;
        const f32x4 a = *reinterpret_cast<const f32x4 *>(act + off);
        f32x4 g = *reinterpret_cast<f32x4 *>(d + off);
#pragma unroll
        for (int e = 0; e < 4; ++e) g[e] = a[e] > 0.f ? g[e] : 0.f;
        *reinterpret_cast<f32x4 *>(d + off) = g;
    }
}

hipError_t launch_slice_gate(const float *act, float *d, long long rows, int Cs, int c_off, int C, hipStream_t stream)
{
    if (rows < 1 || C < 4 || (C & 3) || (Cs & 3) || (c_off & 3) || c_off < 0 || c_off + C > Cs) return hipErrorInvalidValue;
    const long long total = rows * (C / 4);
    const long long blocks = std::min<long long>((total + 255) / 256, 256 * 16);
    slice_gate_kernel<<<dim3((unsigned)blocks), dim3(256), 0, stream>>>(act, d, rows, Cs, c_off, C / 4);
    return hipGetLastError();
}

}  // namespace vstab
