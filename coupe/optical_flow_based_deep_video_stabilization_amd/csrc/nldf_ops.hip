// Small kernels of the NLDF saliency head (NLDF.py:24-134; SURVEY.md 8a row N1, tertiary: the
// reference never instantiates it) and its VGG16 front end (max pool, preprocessing, conv1_1).  The other convolutions run on the MFMA kernel.
#include "vstab_internal.h"

namespace vstab {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// Contrast_Layer (NLDF.py:131-134): x - avg_pool3x3(VALID) of x padded by 1 with tf.pad 'SYMMETRIC'
// (for a pad of 1: the edge pixel repeated).  Reads channels [0,C) and writes [c_dst, c_dst+C) of the same
// Cs-wide pixels (the [Fea | Fea_LC] half of a concat buffer).  One thread per 4 channels.
__global__ __launch_bounds__(256) void contrast_kernel(float *__restrict__ buf, int B, int H, int W, int C4, int Cs, int c_dst)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long total = (long long)B * H * W * C4;
    if (idx >= total) return;
    const int c = (int)(idx % C4);
    const long long pix = idx / C4;
    const int n = (int)(pix / (H * W));
    const int rem = (int)(pix - (long long)n * H * W);
    const int y = rem / W, x = rem - y * W;
    const float *b = buf + (long long)n * H * W * Cs + c * 4;
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
    f32x4 o;
    o.x = ctr.x - s.x / 9.0f; o.y = ctr.y - s.y / 9.0f; o.z = ctr.z - s.z / 9.0f; o.w = ctr.w - s.w / 9.0f;
    *reinterpret_cast<f32x4 *>(buf + (long long)pix * Cs + c_dst + c * 4) = o;
}

hipError_t launch_contrast(float *buf, int B, int H, int W, int C, int Cs, int c_dst, hipStream_t stream)
{
    if ((C & 3) || (Cs & 3) || (c_dst & 3) || c_dst < C) return hipErrorInvalidValue;
    const long long total = (long long)B * H * W * (C / 4);
    contrast_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream>>>(buf, B, H, W, C / 4, Cs, c_dst);
    return hipGetLastError();
}

// Score = Local_Score + Global_Score (broadcast over the image), Prob = softmax(Score)[..., 0] (NLDF.py:73-77)
__global__ __launch_bounds__(256) void nldf_score_kernel(const float *__restrict__ local2, const float *__restrict__ global2,
                                                         int B, int npix, float *__restrict__ score, float *__restrict__ prob)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)B * npix) return;
    const int n = (int)(idx / npix);
    const float s0 = local2[2 * idx] + global2[2 * n], s1 = local2[2 * idx + 1] + global2[2 * n + 1];
    if (score) { score[2 * idx] = s0; score[2 * idx + 1] = s1; }
    const float m = fmaxf(s0, s1);
    const float e0 = expf(s0 - m), e1 = expf(s1 - m);
    prob[idx] = e0 / (e0 + e1);
}

hipError_t launch_nldf_score(const float *local2, const float *global2, int B, int npix, float *score, float *prob, hipStream_t stream)
{
    const long long total = (long long)B * npix;
    nldf_score_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream>>>(local2, global2, B, npix, score, prob);
    return hipGetLastError();
}

// tf.nn.max_pool(ksize 2, strides 2, SAME) (vgg16.py:51-53): out = ceil(n/2); the window's taps beyond
// the bottom/right edge do not take part.  One thread per 4 output channels.
__global__ __launch_bounds__(256) void maxpool2x2_kernel(const float *__restrict__ x, int B, int H, int W, int C4,
                                                         float *__restrict__ out, int oh, int ow)
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
    const bool y1ok = y0 + 1 < H, x1ok = x0 + 1 < W;
    const f32x4 *b = reinterpret_cast<const f32x4 *>(x) + (long long)n * H * W * C4 + c;
    f32x4 m = b[((long long)y0 * W + x0) * C4];
    if (x1ok) { const f32x4 v = b[((long long)y0 * W + x0 + 1) * C4]; m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w); }
    if (y1ok) {
        const f32x4 v = b[((long long)(y0 + 1) * W + x0) * C4]; m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
        if (x1ok) { const f32x4 u = b[((long long)(y0 + 1) * W + x0 + 1) * C4]; m.x = fmaxf(m.x, u.x); m.y = fmaxf(m.y, u.y); m.z = fmaxf(m.z, u.z); m.w = fmaxf(m.w, u.w); }
    }
    reinterpret_cast<f32x4 *>(out)[idx] = m;
}

hipError_t launch_maxpool2x2(const float *x, int B, int H, int W, int C, float *out, hipStream_t stream)
{
    if (C & 3) return hipErrorInvalidValue;
    const int oh = (H + 1) / 2, ow = (W + 1) / 2;
    const long long total = (long long)B * oh * ow * (C / 4);
    maxpool2x2_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream>>>(x, B, H, W, C / 4, out, oh, ow);
    return hipGetLastError();
}

// NLDF.py:29: input * 255 - VGG_MEAN (per channel)
struct Mean4 { float m[4]; };
__global__ __launch_bounds__(256) void scale_shift_kernel(const float *__restrict__ x, long long n, int C, float scale, Mean4 mean,
                                                          float *__restrict__ out)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const int c = (int)(idx % C);
    out[idx] = x[idx] * scale - mean.m[c];
}

// VGG16's first layer (conv1_1, vgg16.py:29: 3x3 SAME on the 3-channel image -> 64 channels, ReLU): K = 27 is a single padded
// K-tile of the MFMA kernel, whose time is then its 4-byte scattered epilogue (1.2 TB/s on the 2.1 GB it writes at 4 x 1080p).  This
// layer is an HBM-bound WRITE, so it gets a plain kernel shaped for the store: 16 lanes per pixel, one float4 of output channels
// each (256 contiguous bytes per pixel), four pixels of a row per thread so that each filter chunk is read from LDS once for the
// four; the 3x6x3 input window comes through L1 (the 16 lanes of a pixel group hit the same addresses), filter + bias sit in LDS.  W: HWIO [3][3][3][cout], cout % 4 == 0, cout <= 64.
__global__ __launch_bounds__(256) void conv3x3_rgb_kernel(const float *__restrict__ x, int B, int H, int W, const float *__restrict__ Wf,
                                                          const float *__restrict__ bias, int cout, int relu, float *__restrict__ out)
{
    __shared__ f32x4 sW[27 * 16];
    __shared__ f32x4 sB[16];
    const int q4 = cout >> 2;
    for (int i = threadIdx.x; i < 27 * q4; i += 256) sW[(i / q4) * 16 + (i % q4)] = *reinterpret_cast<const f32x4 *>(Wf + (long long)(i / q4) * cout + (i % q4) * 4);
    if (threadIdx.x < q4) sB[threadIdx.x] = *reinterpret_cast<const f32x4 *>(bias + threadIdx.x * 4);
    __syncthreads();
    // a thread: 4 consecutive pixels of a row x one float4 of output channels (the filter chunk is read once for the four)
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const int q = (int)(idx & 15);
    const long long grp = idx >> 4;
    const int WQ = (W + 3) >> 2;
    if (grp >= (long long)B * H * WQ || q >= q4) return;
    const int n = (int)(grp / ((long long)H * WQ));
    const int rem = (int)(grp - (long long)n * H * WQ);
    const int y = rem / WQ, x0 = (rem - y * WQ) * 4;
    const float *xb = x + (long long)n * H * W * 3;
    f32x4 acc[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) acc[p] = sB[q];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = y + ky - 1;
        const bool yok = (unsigned)iy < (unsigned)H;
        float v[6][3];                                   // input columns x0-1 .. x0+4 of this row
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const int ix = x0 + j - 1;
            const bool ok = yok && (unsigned)ix < (unsigned)W;
            const float *px = xb + ((long long)iy * W + ix) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) v[j][c] = ok ? px[c] : 0.f;
        }
#pragma unroll
        for (int kx = 0; kx < 3; ++kx)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const f32x4 w = sW[((ky * 3 + kx) * 3 + c) * 16 + q];
#pragma unroll
                for (int p = 0; p < 4; ++p) acc[p] += v[p + kx][c] * w;
            }
    }
    float *o = out + (((long long)n * H + y) * W + x0) * cout + q * 4;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        if (x0 + p >= W) break;
        f32x4 r = acc[p];
        if (relu) {
#pragma unroll
            for (int e = 0; e < 4; ++e) r[e] = fmaxf(r[e], 0.f);
        }
        *reinterpret_cast<f32x4 *>(o + (long long)p * cout) = r;
    }
}

hipError_t launch_conv3x3_rgb(const float *x, int B, int H, int W, const float *Wf, const float *bias, int cout, int relu, float *out,
                              hipStream_t stream)
{
    if ((cout & 3) || cout > 64 || cout < 4) return hipErrorInvalidValue;
    const long long n = (long long)B * H * ((W + 3) / 4) * 16;
    conv3x3_rgb_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream>>>(x, B, H, W, Wf, bias, cout, relu, out);
    return hipGetLastError();
}

hipError_t launch_scale_shift(const float *x, long long npix, int C, float scale, const float *mean4, float *out, hipStream_t stream)
{
    if (C < 1 || C > 4) return hipErrorInvalidValue;
    Mean4 m{};
    for (int c = 0; c < C; ++c) m.m[c] = mean4[c];
    const long long n = npix * C;
    scale_shift_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream>>>(x, n, C, scale, m, out);
    return hipGetLastError();
}

}  // namespace vstab
