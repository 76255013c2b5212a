// The training loader's batch assembly (data_loader.py: _read_frame :203-206 + read_dataset :132-169, main:179-184): nine frames of a
// clip, each  cv2.resize(cvtColor(imread, BGR2RGB) / 255., (W, H)), laid out as the three tensors train() feeds -- straight from the
// clip's 8-bit frames in HBM, so a batch is never built on the host and never crosses the bus as 189 MB of fp32.
#include "vstab_internal.h"

namespace vstab {

// cv2.resize with the default INTER_LINEAR on a 64-bit image (`/ 255.` makes the frame float64).  Like resize_u8_kernel and
// resize_f32_to_u8_kernel (clip_ops.hip) this restates OpenCV's published generic path (imgproc/resize.cpp) and is NOT pinned against
// cv2 itself, which is not installed here:
//   scale = 1. / ((double)dn / sn);  fx = (float)((dx+0.5)*scale - 0.5) [product and difference in double];  sx = floor(fx);  fx -= sx;
//   sx < 0 -> (0, fx = 0);  sx >= sn-1 -> (sn-1, fx = 0);  the coefficients stay FLOAT: a0 = 1.f - fx, a1 = fx  (HResizeLinear<double,double,float>)
//   R = S[x0]*a0 + S[x1]*a1  then  D = b0*R[y0] + b1*R[y1], every product and sum one IEEE double operation (the build passes
//   -ffp-contract=off), S = u/255. the IEEE double quotient; the fp32 placeholder rounds D once (main:179-181).
// What pins it: tests/data_loader_ref.py restates the same arithmetic in NumPy float64 and the kernel equals it bit for bit
// (tests/test_gpu_data_loader.py); that restatement is itself held to known answers, cv_resize_f32 and an independent scipy bilinear.
// dn == sn gives a0 = 1, a1 = 0 on every tap, so D == S exactly: cv2's copy for dsize == ssize needs no path of its own.
struct TapD { int i0, i1; double a0, a1; };
__device__ __forceinline__ TapD cv_tap_f(int d, double scale, int sn)
{
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (s < 0) { f = 0.f; s = 0; }
    if (s >= sn - 1) { f = 0.f; s = sn - 1; }
    TapD t;
    t.i0 = s; t.i1 = min(s + 1, sn - 1);
    t.a0 = (double)(1.f - f);
    t.a1 = (double)f;
    return t;
}

// u / 255. for the 256 byte values, divided by the HOST compiler (constant evaluation is IEEE): part of the code object, no upload.
struct Lut255 { double v[256]; };
static constexpr Lut255 make_lut255()
{
    Lut255 t{};
    for (int i = 0; i < 256; ++i) t.v[i] = (double)i / 255.;
    return t;
}
__device__ const Lut255 k_lut255 = make_lut255();

// The samples of one launch travel by value in the kernel arguments (as Slots9 does): no copy to the device, nothing to synchronise.
struct TrainBatchIdx { int row[TRAIN_BATCH_LAUNCH_SAMPLES]; int frame[TRAIN_BATCH_LAUNCH_SAMPLES][9]; };

// A workgroup owns 256 consecutive pixels of ONE output row of the batch: 27 648 contiguous bytes of feats and 3 072 each of gtstab and
// unstab.  As in assemble_input_kernel (clip_ops.hip: 4-byte stores 108 bytes apart ran at 1.2 TB/s) the values go through LDS and
// leave as 16-byte stores.  A sample's first float is 16-byte aligned only when H*W is a multiple of 4, so each run is placed in LDS
// at the offset its first float has inside its 16-byte quad (`shift`): aligned LDS quads are then aligned global quads, and the up to
// three floats before the first and after the last full quad are stored one by one.  [pixel][27] and [pixel][3] are odd strides.
typedef float f32x4_tb __attribute__((ext_vector_type(4)));
struct TrainBatchLds {
    double lut[256];
    float f[256 * 27 + 4];
    float g[256 * 3 + 4];
    float u[256 * 3 + 4];
};
__device__ __forceinline__ int quad_shift(const float *p) { return (int)(((unsigned long long)p >> 2) & 3); }
// v[shift + k] -> run[k], k < nfl; shift == quad_shift(run)
__device__ __forceinline__ void store_run(const float *v, float *__restrict__ run, int shift, int nfl)
{
    float *o = run - shift;
    const int end = shift + nfl;
    for (int e = threadIdx.x * 4; e < end; e += 1024) {
        if (e >= shift && e + 4 <= end) *reinterpret_cast<f32x4_tb *>(o + e) = *reinterpret_cast<const f32x4_tb *>(v + e);
        else for (int i = 0; i < 4; ++i) if (e + i >= shift && e + i < end) o[e + i] = v[e + i];
    }
}

// grid (ceil(H*W / 256), samples of this launch)
__global__ __launch_bounds__(256) void assemble_train_batch_kernel(const unsigned char *__restrict__ stab, const unsigned char *__restrict__ unstab,
                                                                   int sh, int sw, TrainBatchIdx idx, float *__restrict__ feats,
                                                                   float *__restrict__ gtstab, float *__restrict__ unstab_out, int H, int W,
                                                                   double scale_x, double scale_y)
{
    __shared__ __attribute__((aligned(16))) TrainBatchLds L;
    L.lut[threadIdx.x] = k_lut255.v[threadIdx.x];
    const int s = blockIdx.y;
    const int hw = H * W;                                                       // < 2^31: checked by the caller
    const int p0 = blockIdx.x * 256, p = p0 + threadIdx.x;
    const int npx = min(256, hw - p0);
    const long long first = (long long)idx.row[s] * hw + p0;                    // first pixel of the block in [B*H*W]
    float *of = feats + first * 27, *og = gtstab + first * 3, *ou = unstab_out + first * 3;
    const int sf = quad_shift(of), sg = quad_shift(og), su = quad_shift(ou);
    __syncthreads();
    if (p < hw) {
        const int dy = p / W, dx = p - dy * W;
        const TapD X = cv_tap_f(dx, scale_x, sw), Y = cv_tap_f(dy, scale_y, sh);
        const long long frame_bytes = (long long)sh * sw * 3;
        const long long o00 = ((long long)Y.i0 * sw + X.i0) * 3, o01 = ((long long)Y.i0 * sw + X.i1) * 3;
        const long long o10 = ((long long)Y.i1 * sw + X.i0) * 3, o11 = ((long long)Y.i1 * sw + X.i1) * 3;
        // the ten frames of a sample share the pixel's taps and coefficients
        auto resize3 = [&](const unsigned char *fr, float *o) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double R0 = L.lut[fr[o00 + c]] * X.a0 + L.lut[fr[o01 + c]] * X.a1;
                const double R1 = L.lut[fr[o10 + c]] * X.a0 + L.lut[fr[o11 + c]] * X.a1;
                o[c] = (float)(Y.a0 * R0 + Y.a1 * R1);
            }
        };
        float *f = L.f + sf + threadIdx.x * 27;
#pragma unroll
        for (int j = 0; j < 8; ++j) resize3(stab + (long long)idx.frame[s][j] * frame_bytes, f + 3 * j);
        const long long last = (long long)idx.frame[s][8] * frame_bytes;
        float *u = L.u + su + threadIdx.x * 3;
        resize3(unstab + last, u);
        f[24] = u[0]; f[25] = u[1]; f[26] = u[2];                               // concat([stab_image, unstab_image], 3), main:184
        resize3(stab + last, L.g + sg + threadIdx.x * 3);
    }
    __syncthreads();
    store_run(L.f, of, sf, npx * 27);
    store_run(L.g, og, sg, npx * 3);
    store_run(L.u, ou, su, npx * 3);
}

hipError_t launch_assemble_train_batch(const unsigned char *stab, const unsigned char *unstab, int sh, int sw, const int *rows, const int *frame_idx,
                                       int n, float *feats, float *gtstab, float *unstab_out, int H, int W, hipStream_t stream)
{
    const double scale_x = 1.0 / ((double)W / (double)sw), scale_y = 1.0 / ((double)H / (double)sh);
    const unsigned blocks = (unsigned)(((long long)H * W + 255) / 256);
    for (int i0 = 0; i0 < n; i0 += TRAIN_BATCH_LAUNCH_SAMPLES) {
        const int ns = n - i0 < TRAIN_BATCH_LAUNCH_SAMPLES ? n - i0 : TRAIN_BATCH_LAUNCH_SAMPLES;
        TrainBatchIdx idx = {};
        for (int i = 0; i < ns; ++i) {
            idx.row[i] = rows[i0 + i];
            for (int j = 0; j < 9; ++j) idx.frame[i][j] = frame_idx[(size_t)(i0 + i) * 9 + j];
        }
        assemble_train_batch_kernel<<<dim3(blocks, (unsigned)ns), dim3(256), 0, stream>>>(stab, unstab, sh, sw, idx, feats, gtstab, unstab_out, H, W,
                                                                                         scale_x, scale_y);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace vstab
