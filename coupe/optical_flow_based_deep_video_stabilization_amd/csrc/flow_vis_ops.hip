// Kernels of flow_vis.py: the Middlebury colour code of a dense flow field (flow_to_image, compute_color and make_color_wheel at the
// end of each of the reference's main scripts, main_flownetS_pyramid.py:824-957).
//
//   flow [B,H,W,2] fp32  ->  img [B,H,W,3] uint8 (and, when asked for, anglemap [B,H,W,3] uint8)
//
// Two launches, stream-ordered, no atomics: two runs give the same bytes.
//
//   flow_maxrad_partial_kernel  (skipped when the caller gives the radii) grid (P, B): the largest u*u + v*v of a slice of one
//       sample, unknown pixels (|u| or |v| > 1e7) counting as (0,0) and NaN pixels left out; float4 (two pixels) loads after a head
//       of at most one pixel, a grid-stride maximum per thread, a cross-lane maximum per wave, one float per workgroup.
//   flow_colour_kernel  grid (ceil(groups / 1024), B): each workgroup first takes the maximum of its sample's P partials and ONE
//       square root (sqrt is monotone and correctly rounded, so this is the reference's max(sqrt(..))), then every thread colours
//       groups of four pixels: 32 B of flow in, three dwords of img (and of anglemap) out.  A sample's first pixels up to the 4-byte
//       boundary of img and its last pixels go one by one.
//
// Per pixel the arithmetic and its order are those of the reference under the NumPy of its day, fp32 up to the wheel lookup and
// fp64 from there (the float64 wheel promotes everything it meets); the colour jumps at radius 1 and at the +-pi seam, so a
// differently rounded radius or a lost sign of zero would change a pixel visibly:
//   d = maxrad > 0 ? maxrad : 2^-52;  un = u / d, vn = v / d             (unknown and NaN pixels: u = v = +0)
//   rad = sqrtf(un*un + vn*vn)                                           (not contracted: the build passes -ffp-contract=off)
//   a = atan2f(-vn, -un) / (float)pi                                     (real negations: v = +0 gives -0)
//   fk = (a + 1) / 2 * 54 + 1;  k0 = floor(fk);  k1 = k0 + 1, 56 -> 1;  f = fk - k0
//   col = (1 - f) * wheel[k0-1]/255 + f * wheel[k1-1]/255                (fp64 from here)
//   col = rad <= 1 ? 1 - rad * (1 - col) : 0.75 * col;  byte = floor(255 * col)
//   anglemap byte = trunc(a * 127 + 128)                                 (fp32)
// Unknown and NaN pixels are black in img; their anglemap byte is that of (+0, +0), which is 1, as in the reference.
#include "vstab_internal.h"

namespace vstab {

namespace {

constexpr int NCOLS = 55;
struct ColourWheel { double c[NCOLS][3]; };          // wheel / 255, correctly rounded doubles (what numpy's tmp[k] / 255 gives)

// make_color_wheel: six segments of lengths 15, 6, 4, 11, 13, 6; in each one channel stays at 255 and another ramps up as
// floor(255 i / n) or down as 255 - floor(255 i / n)
constexpr ColourWheel make_wheel()
{
    ColourWheel w{};
    constexpr int len[6] = {15, 6, 4, 11, 13, 6};
    constexpr int full[6] = {0, 1, 1, 2, 2, 0};      // RY, YG, GC, CB, BM, MR: the channel held at 255 ...
    constexpr int ramp[6] = {1, 0, 2, 1, 0, 2};      // ... and the one that moves,
    constexpr bool down[6] = {false, true, false, true, false, true};
    int row = 0;
    for (int s = 0; s < 6; ++s)
        for (int i = 0; i < len[s]; ++i, ++row) {
            const int r = 255 * i / len[s];          // floor: the operands are non-negative
            w.c[row][full[s]] = 255.0 / 255.0;
            w.c[row][ramp[s]] = (double)(down[s] ? 255 - r : r) / 255.0;
        }
    return w;
}

__constant__ ColourWheel c_wheel = make_wheel();

constexpr float UNKNOWN_FLOW = 1e7f;
constexpr float PI_F = 3.14159265358979323846f;      // (float)np.pi
constexpr double EPS64 = 2.220446049250313e-16;      // np.finfo(float).eps = 2^-52, exact in fp32 too

__device__ __forceinline__ bool flow_undefined(float u, float v)
{
    return fabsf(u) > UNKNOWN_FLOW || fabsf(v) > UNKNOWN_FLOW || u != u || v != v;
}

// u*u + v*v of a pixel as pass 1 counts it: 0 for an unknown pixel (the reference zeroes it) and for a NaN pixel (left out: the
// running maximum starts at 0)
__device__ __forceinline__ float flow_sq(float u, float v)
{
    return flow_undefined(u, v) ? 0.f : u * u + v * v;
}

__device__ __forceinline__ float block_max_256(float v, float *red)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// grid (P, B), 256 threads.  partial [B][P]: the largest u*u + v*v in workgroup x's share of sample y
__global__ __launch_bounds__(256) void flow_maxrad_partial_kernel(const float *__restrict__ flow, int HW, float *__restrict__ partial)
{
    __shared__ float red[4];
    const int P = gridDim.x, b = blockIdx.y;
    const float *p = flow + (size_t)b * HW * 2;                         // 8-byte aligned (the entry point checks the base)
    const int head = (((uintptr_t)p) & 15) ? 1 : 0;                      // pixels before the first 16-byte boundary
    const int pairs = HW > head ? (HW - head) / 2 : 0;
    const int t = blockIdx.x * 256 + threadIdx.x, stride = P * 256;
    float m = 0.f;
    const float4 *p4 = reinterpret_cast<const float4 *>(p + 2 * head);
#pragma unroll 4
    for (int i = t; i < pairs; i += stride) {
        const float4 q = p4[i];
        m = fmaxf(m, fmaxf(flow_sq(q.x, q.y), flow_sq(q.z, q.w)));
    }
    if (t == 0 && head && HW >= 1) m = fmaxf(m, flow_sq(p[0], p[1]));
    const int done = head + 2 * pairs;                                   // at most one pixel is left
    if (t == 1 && done < HW) m = fmaxf(m, flow_sq(p[2 * done], p[2 * done + 1]));
    m = block_max_256(m, red);
    if (threadIdx.x == 0) partial[(size_t)b * P + blockIdx.x] = m;
}

struct PixelBytes { unsigned rgb, ang; };            // r | g << 8 | b << 16, and the anglemap byte

__device__ __forceinline__ PixelBytes colour_pixel(float u, float v, float d, const double (*wheel)[3])
{
    const bool undefined = flow_undefined(u, v);
    if (undefined) { u = 0.f; v = 0.f; }
    const float un = u / d, vn = v / d;
    const float rad = sqrtf(un * un + vn * vn);
    const float a = atan2f(-vn, -un) / PI_F;
    const float fk = (a + 1.f) / 2.f * (float)(NCOLS - 1) + 1.f;
    const float k0f = floorf(fk);
    int k0 = (int)k0f;
    k0 = k0 < 1 ? 1 : (k0 > NCOLS ? NCOLS : k0);                         // 1..55 whenever |a| <= 1; keeps the table read in bounds
    const int k1 = k0 == NCOLS ? 1 : k0 + 1;
    const double f = (double)(fk - k0f);                                 // exact in fp32
    PixelBytes out;
    out.ang = (unsigned)(a * 127.f + 128.f);
    out.rgb = 0;
    if (!undefined) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            double col = (1.0 - f) * wheel[k0 - 1][c] + f * wheel[k1 - 1][c];
            col = rad <= 1.f ? 1.0 - (double)rad * (1.0 - col) : col * 0.75;
            out.rgb |= ((unsigned)floor(255.0 * col) & 255u) << (8 * c);
        }
    }
    return out;
}

__device__ __forceinline__ void store_pixel(unsigned char *dst, unsigned rgb)
{
    dst[0] = (unsigned char)rgb;
    dst[1] = (unsigned char)(rgb >> 8);
    dst[2] = (unsigned char)(rgb >> 16);
}

// four pixels' 24-bit values as the three dwords of their 12 bytes
__device__ __forceinline__ void pack4(const unsigned (&p)[4], unsigned (&w)[3])
{
    w[0] = p[0] | (p[1] << 24);
    w[1] = (p[1] >> 8) | (p[2] << 16);
    w[2] = (p[2] >> 16) | (p[3] << 8);
}

constexpr int COLOUR_ITERS = 4;                      // groups of four pixels per thread

// grid (ceil(groups / (256 * COLOUR_ITERS)) or 1, B), 256 threads.  partial [B][P] from the kernel above, or maxrad_in [B]
__global__ __launch_bounds__(256) void flow_colour_kernel(const float *__restrict__ flow, int HW, const float *__restrict__ maxrad_in,
                                                          const float *__restrict__ partial, int P, unsigned char *__restrict__ img,
                                                          unsigned char *__restrict__ ang, float *__restrict__ maxrad_out)
{
    __shared__ float red[4];
    __shared__ double wheel[NCOLS][3];
    const int b = blockIdx.y, t = threadIdx.x;
    if (t < NCOLS * 3) (&wheel[0][0])[t] = (&c_wheel.c[0][0])[t];
    float maxrad;
    if (maxrad_in) {
        maxrad = maxrad_in[b];
        __syncthreads();
    } else {
        maxrad = sqrtf(block_max_256(t < P ? partial[(size_t)b * P + t] : 0.f, red));      // its barrier covers the wheel too
    }
    if (maxrad_out && blockIdx.x == 0 && t == 0) maxrad_out[b] = maxrad;
    const float d = maxrad > 0.f ? maxrad : (float)EPS64;

    const float *fl = flow + (size_t)b * HW * 2;
    unsigned char *im = img + (size_t)b * HW * 3;
    unsigned char *an = ang ? ang + (size_t)b * HW * 3 : nullptr;
    // pixel h of the sample is the first whose img bytes start on a 4-byte boundary: (im + 3h) % 4 == 0  <=>  h == im % 4
    int head = (int)(((uintptr_t)im) & 3);
    if (head > HW) head = HW;
    const int groups = (HW - head) / 4;
    const bool flow16 = ((((uintptr_t)fl) + 8 * (size_t)head) & 15) == 0;
    const bool ang_words = an && ((((uintptr_t)an) & 3) == (((uintptr_t)im) & 3));

    for (int it = 0; it < COLOUR_ITERS; ++it) {
        const int g = (blockIdx.x * COLOUR_ITERS + it) * 256 + t;
        if (g >= groups) break;
        const int px = head + 4 * g;
        float uv[8];
        if (flow16) {
            const float4 q0 = *reinterpret_cast<const float4 *>(fl + 2 * (size_t)px);
            const float4 q1 = *reinterpret_cast<const float4 *>(fl + 2 * (size_t)px + 4);
            uv[0] = q0.x; uv[1] = q0.y; uv[2] = q0.z; uv[3] = q0.w; uv[4] = q1.x; uv[5] = q1.y; uv[6] = q1.z; uv[7] = q1.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float2 q = *reinterpret_cast<const float2 *>(fl + 2 * (size_t)(px + j));
                uv[2 * j] = q.x; uv[2 * j + 1] = q.y;
            }
        }
        unsigned rgb[4], gray[4], w[3];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const PixelBytes pb = colour_pixel(uv[2 * j], uv[2 * j + 1], d, wheel);
            rgb[j] = pb.rgb;
            gray[j] = pb.ang * 0x010101u;
        }
        pack4(rgb, w);
        unsigned *iw = reinterpret_cast<unsigned *>(im + 3 * (size_t)px);
        iw[0] = w[0]; iw[1] = w[1]; iw[2] = w[2];
        if (ang_words) {
            pack4(gray, w);
            unsigned *aw = reinterpret_cast<unsigned *>(an + 3 * (size_t)px);
            aw[0] = w[0]; aw[1] = w[1]; aw[2] = w[2];
        } else if (an) {
#pragma unroll
            for (int j = 0; j < 4; ++j) store_pixel(an + 3 * (size_t)(px + j), gray[j]);
        }
    }
    // the head and the tail, at most three pixels each, one thread per pixel of workgroup 0
    if (blockIdx.x == 0) {
        const int tail0 = head + 4 * groups, ntail = HW - tail0;
        const int px = t < head ? t : tail0 + (t - head);
        if (t < head + ntail) {
            const PixelBytes pb = colour_pixel(fl[2 * (size_t)px], fl[2 * (size_t)px + 1], d, wheel);
            store_pixel(im + 3 * (size_t)px, pb.rgb);
            if (an) store_pixel(an + 3 * (size_t)px, pb.ang * 0x010101u);
        }
    }
}

}  // namespace

int flow_vis_partials(int H, int W)
{
    const long long hw = (long long)H * W;
    const long long p = (hw + FLOW_VIS_SLICE - 1) / FLOW_VIS_SLICE;
    return (int)(p < 1 ? 1 : (p > FLOW_VIS_MAX_PARTIALS ? FLOW_VIS_MAX_PARTIALS : p));
}

hipError_t launch_flow_to_image(const float *flow, int B, int H, int W, const float *maxrad_in, unsigned char *img, unsigned char *anglemap,
                                float *maxrad_out, float *partial, hipStream_t stream)
{
    const int HW = H * W, P = flow_vis_partials(H, W);
    if (!maxrad_in) {
        hipLaunchKernelGGL(flow_maxrad_partial_kernel, dim3(P, B), dim3(256), 0, stream, flow, HW, partial);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    const int groups = HW / 4, per_block = 256 * COLOUR_ITERS;
    const int gx = groups > 0 ? (groups + per_block - 1) / per_block : 1;
    hipLaunchKernelGGL(flow_colour_kernel, dim3(gx, B), dim3(256), 0, stream, flow, HW, maxrad_in, partial, P, img, anglemap, maxrad_out);
    return hipGetLastError();
}

}  // namespace vstab
