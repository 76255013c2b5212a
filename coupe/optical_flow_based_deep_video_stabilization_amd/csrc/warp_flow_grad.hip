// Backward of tf_warp (main:70-130, "main" = main_flownetS_pyramid_noprevloss_dataloader.py) and of get_pixel_value (main:44-68):
// what TensorFlow's autodiff yields for the forward of flow_ops.hip, with the forward's own corner and weight arithmetic
// (warp_taps.h), so every truncation and clip decision is shared with it.
//
// With x = xx + fx, y = yy + fy, the clipped corners x0, x1, y0, y1 and their float casts (a = (y0,x0), b = (y1,x0), c = (y0,x1),
// d = (y1,x1)) and dout the gradient of the warped frame:
//   d flow  The corner indices come from integer casts and carry no gradient; the flow enters through the four weights only:
//             d_fx = sum_c dout_c [(y1f - y)(Ic - Ia) + (y - y0f)(Id - Ib)]_c,  d_fy = sum_c dout_c [(x1f - x)(Ib - Ia) + (x - x0f)(Id - Ic)]_c
//           (tf_warp_slope, channels in order).  Where both corners of an axis clip to the same border pixel the bracket is exactly
//           0.  One thread per pixel, plain stores, no atomics: bit-reproducible.
//   d img   The gather's adjoint: wa dout -> (y0,x0), wb dout -> (y1,x0), wc dout -> (y0,x1), wd dout -> (y1,x1) with the forward's
//           weights, taken from the clipped corners -- outside the image they are negative or above 1, as in the reference.  Added
//           by fp32 atomics, so the last bits of d img depend on the order in which the contributions arrive; zeroed first unless
//           the caller accumulates.
// A NaN / infinite / huge flow is clamped by tf_warp_taps before the float -> int conversion: its taps are border pixels (row 0 or
// H - 1, or column 0 or W - 1), never out of bounds; what such a pixel adds there, and its own d flow, is NaN or infinite.
//
// Two forms, as the forward has: one thread per pixel over the flat index (any channel count, either output), and for the d flow of
// 3-channel frames the tile skeleton of tile3.h (16 x 32 tile of one sample, 4 x 16 wave patches, XCD-contiguous tile order, one
// 3-dword load per corner and for dout): 1.5x (smooth flows) to 2.6x (random flows) the pixel kernel, 1.03-1.3x the forward's time.
// Either output may be skipped; the d flow-only form has neither atomics nor the memset.
// Measured and dropped (profiles/README.md, "warp backward"): d img on the tile skeleton.  The atomics bound every form that
// writes d img (20-60x the forward), and a 4 x 16 patch puts the four lanes that share a corner into one wave instruction: 0.8x the
// pixel kernel on smooth flows, 1.1-1.2x on random ones.  So a call that wants d img runs the pixel kernel for both outputs.
// Algorithmic bytes per pixel for C = 3: 12 dout + 8 flow read; d flow: + 12 of gathers (the four corners hit in cache as in the
// forward) + 8 written; d img: + four 12-byte atomic read-modify-writes.
#include "vstab_internal.h"
#include "tile3.h"
#include "warp_taps.h"
#include <cstdlib>

namespace vstab {
namespace {

using WarpTile = Tile3<>;

// One pixel, any channel count.  b / di: the sample's frame and its gradient; g: the pixel's dout.
template <bool DIMG, bool DFLOW>
__device__ __forceinline__ f32x2 warp_bwd_point(const float *__restrict__ b, float *di, const float *__restrict__ g, int W, int C, const WarpTaps &t,
                                                const WarpAxes &a)
{
    const long long ia = ((long long)t.y0 * W + t.x0) * C, ib = ((long long)t.y1 * W + t.x0) * C;
    const long long ic = ((long long)t.y0 * W + t.x1) * C, id = ((long long)t.y1 * W + t.x1) * C;
    float gx = 0.f, gy = 0.f;
    for (int c = 0; c < C; ++c) {
        const float gc = g[c];
        if (DFLOW) tf_warp_slope(a, b[ia + c], b[ib + c], b[ic + c], b[id + c], gc, gx, gy);
        if (DIMG) {
            atomicAdd(di + ia + c, t.wa * gc); atomicAdd(di + ib + c, t.wb * gc);
            atomicAdd(di + ic + c, t.wc * gc); atomicAdd(di + id + c, t.wd * gc);
        }
    }
    f32x2 d = {gx, gy};
    return d;
}

template <bool DIMG, bool DFLOW>
__global__ __launch_bounds__(256) void warp_flow_bwd_kernel(const float *__restrict__ img, const float *__restrict__ flow,
                                                            const float *__restrict__ dout, float *d_img, float *__restrict__ d_flow, int B,
                                                            int H, int W, int C)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long total = (long long)B * H * W;
    if (idx >= total) return;
    const int n = (int)(idx / (H * W));
    const int rem = (int)(idx - (long long)n * H * W);
    const int yy = rem / W, xx = rem - yy * W;
    const f32x2 f = reinterpret_cast<const f32x2 *>(flow)[idx];
    const float x = (float)xx + f.x, y = (float)yy + f.y;
    const WarpTaps t = tf_warp_taps(x, y, H, W);
    const long long so = (long long)n * H * W * C;
    const f32x2 d = warp_bwd_point<DIMG, DFLOW>(img + so, DIMG ? d_img + so : nullptr, dout + idx * C, W, C, t, tf_warp_axes(t, x, y));
    if (DFLOW) reinterpret_cast<f32x2 *>(d_flow)[idx] = d;
}

// d flow of 3-channel frames: B H W < 2^31 (host), so a sample's pixel offsets fit an int.  Every load of a thread's PPT pixels is
// issued before any arithmetic, as in warp3_pixels.
__global__ __launch_bounds__(256) void warp3_tile_dflow_kernel(const float *__restrict__ img, const float *__restrict__ flow,
                                                               const float *__restrict__ dout, float *__restrict__ d_flow, int B, int H, int W,
                                                               int tiles_x, int tiles_y)
{
    constexpr int PPT = WarpTile::PPT;
    const WarpTile tile(tiles_x, tiles_y);
    const int n = tile.n;
    const long long HW = (long long)H * W;
    const rgb3 *b = reinterpret_cast<const rgb3 *>(img) + n * HW;
    bool ok[PPT];
    long long po[PPT];
    WarpTaps t[PPT];
    WarpAxes a[PPT];
    rgb3 g[PPT], Ia[PPT], Ib[PPT], Ic[PPT], Id[PPT];
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
        const int yy = tile.y(j), xx = tile.x(j);
        ok[j] = yy < H && xx < W;
        if (!ok[j]) continue;
        po[j] = n * HW + (long long)yy * W + xx;
        const f32x2 f = reinterpret_cast<const f32x2 *>(flow)[po[j]];
        g[j] = reinterpret_cast<const rgb3 *>(dout)[po[j]];
        const float x = (float)xx + f.x, y = (float)yy + f.y;
        t[j] = tf_warp_taps(x, y, H, W);
        a[j] = tf_warp_axes(t[j], x, y);
        Ia[j] = b[t[j].y0 * W + t[j].x0]; Ib[j] = b[t[j].y1 * W + t[j].x0];
        Ic[j] = b[t[j].y0 * W + t[j].x1]; Id[j] = b[t[j].y1 * W + t[j].x1];
    }
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
        if (!ok[j]) continue;
        float gx = 0.f, gy = 0.f;
        tf_warp_slope(a[j], Ia[j].r, Ib[j].r, Ic[j].r, Id[j].r, g[j].r, gx, gy);
        tf_warp_slope(a[j], Ia[j].g, Ib[j].g, Ic[j].g, Id[j].g, g[j].g, gx, gy);
        tf_warp_slope(a[j], Ia[j].b, Ib[j].b, Ic[j].b, Id[j].b, g[j].b, gx, gy);
        const f32x2 d = {gx, gy};
        reinterpret_cast<f32x2 *>(d_flow)[po[j]] = d;
    }
}

// Adjoint of get_pixel_value_kernel: dout[b,h,w,:] added to d_img[b, clip(y), clip(x), :] (the forward's clipping) by fp32 atomics
__global__ __launch_bounds__(256) void get_pixel_value_bwd_kernel(const float *__restrict__ dout, const int32_t *__restrict__ x,
                                                                  const int32_t *__restrict__ y, float *d_img, int B, int H, int W, int C, int Hi,
                                                                  int Wi)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long total = (long long)B * H * W;
    if (idx >= total) return;
    const int n = (int)(idx / (H * W));
    const int xi = min(max(x[idx], 0), Wi - 1), yi = min(max(y[idx], 0), Hi - 1);
    float *o = d_img + (((long long)n * Hi + yi) * Wi + xi) * C;
    const float *g = dout + idx * C;
    for (int c = 0; c < C; ++c) atomicAdd(o + c, g[c]);
}

template <bool DIMG, bool DFLOW>
hipError_t launch_bwd(const float *img, const float *flow, const float *dout, int B, int H, int W, int C, float *d_img, float *d_flow, bool tile,
                      hipStream_t stream)
{
    const long long total = (long long)B * H * W;
    int tx, ty;
    dim3 grid;
    if (tile && !DIMG && C == 3 && WarpTile::plan(B, H, W, total, tx, ty, grid))
        warp3_tile_dflow_kernel<<<grid, dim3(256), 0, stream>>>(img, flow, dout, d_flow, B, H, W, tx, ty);
    else
        warp_flow_bwd_kernel<DIMG, DFLOW><<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream>>>(img, flow, dout, d_img, d_flow, B, H, W, C);
    return hipGetLastError();
}
}  // namespace

// d_img and d_flow nullable (not both: the caller's check); H * W < 2^31 and (B H W + 255) / 256 < 2^32 (the caller's check)
hipError_t launch_warp_flow_backward(const float *img, const float *flow, const float *dout, int B, int H, int W, int C, float *d_img,
                                     float *d_flow, int accumulate_img, hipStream_t stream)
{
    // A/B switch of bench_warp_grad.py: the d flow of 3-channel frames through the one-thread-per-pixel kernel too.  Read per call (the
    // benchmark times both forms in one process).
    const bool tile = getenv("VSTAB_WARP_BWD_NO_TILE") == nullptr;
    if (d_img && !accumulate_img) {
        const hipError_t e = hipMemsetAsync(d_img, 0, (size_t)B * H * W * C * sizeof(float), stream);
        if (e != hipSuccess) return e;
    }
    if (d_img && d_flow) return launch_bwd<true, true>(img, flow, dout, B, H, W, C, d_img, d_flow, tile, stream);
    if (d_img) return launch_bwd<true, false>(img, flow, dout, B, H, W, C, d_img, nullptr, tile, stream);
    return launch_bwd<false, true>(img, flow, dout, B, H, W, C, nullptr, d_flow, tile, stream);
}

hipError_t launch_get_pixel_value_backward(const float *dout, const int32_t *x, const int32_t *y, float *d_img, int B, int H, int W, int C,
                                           int Hi, int Wi, int accumulate, hipStream_t stream)
{
    if (!accumulate) {
        const hipError_t e = hipMemsetAsync(d_img, 0, (size_t)B * Hi * Wi * C * sizeof(float), stream);
        if (e != hipSuccess) return e;
    }
    const long long total = (long long)B * H * W;
    get_pixel_value_bwd_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream>>>(dout, x, y, d_img, B, H, W, C, Hi, Wi);
    return hipGetLastError();
}

}  // namespace vstab
