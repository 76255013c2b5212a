// tf_warp's per-pixel arithmetic (main:70-130), stated once for the forward kernels (flow_ops.hip) and the backward kernels
// (warp_flow_grad.hip): the corners and weights of a sample point, the blend, and the slope of the blend in the sample point.
// Corners by float->int truncation toward zero, all four clipped into the image, weights from the CLIPPED corners (A.6).
// Device code only; built with -ffp-contract=off, so every product and sum below is its own fp32 rounding.
#pragma once

namespace vstab {

// the four corners (a = (y0,x0), b = (y1,x0), c = (y0,x1), d = (y1,x1)) and weights of the sample point (x, y): the one statement
// of tf_warp's arithmetic, for the pixel kernel and every tile kernel
struct WarpTaps { int x0, x1, y0, y1; float wa, wb, wc, wd; };
__device__ __forceinline__ WarpTaps tf_warp_taps(float x, float y, int H, int W)
{
    // Clamp BEFORE the conversion: float->int of an out-of-range value and x0 + 1 at INT_MAX are
    // undefined in C++ (the optimiser folds the clips below around them and a NaN/inf flow then
    // indexes out of bounds).  Inside [-2, W] nothing changes; outside, both corners still end
    // up clipped to the same border pixel exactly as in the reference.
    int x0 = (int)fminf(fmaxf(x, -2.f), (float)W), y0 = (int)fminf(fmaxf(y, -2.f), (float)H);
    int x1 = x0 + 1, y1 = y0 + 1;
    WarpTaps t;
    t.x0 = min(max(x0, 0), W - 1); t.x1 = min(max(x1, 0), W - 1);
    t.y0 = min(max(y0, 0), H - 1); t.y1 = min(max(y1, 0), H - 1);
    const float x0f = (float)t.x0, x1f = (float)t.x1, y0f = (float)t.y0, y1f = (float)t.y1;
    t.wa = (x1f - x) * (y1f - y); t.wb = (x1f - x) * (y - y0f);
    t.wc = (x - x0f) * (y1f - y); t.wd = (x - x0f) * (y - y0f);
    return t;
}
__device__ __forceinline__ float tf_warp_blend(const WarpTaps &t, float Ia, float Ib, float Ic, float Id)
{
    return ((t.wa * Ia + t.wb * Ib) + t.wc * Ic) + t.wd * Id;      // tf.add_n order
}

// ---- what TF's autodiff gives for the blend's dependence on the sample point.  The corner indices come from integer casts and
// carry no gradient; (x, y) enters through the four weights only:
//   d out / d x = (y1f - y)(Ic - Ia) + (y - y0f)(Id - Ib),   d out / d y = (x1f - x)(Ib - Ia) + (x - x0f)(Id - Ic)
// with the float casts of the CLIPPED corners.  Where both corners of an axis clip to the same border pixel the two taps of each
// difference are one address and the slope along that axis is exactly 0.
struct WarpAxes { float x1, x0, y1, y0; };       // x1f - x, x - x0f, y1f - y, y - y0f: the factors of tf_warp_taps' weights
__device__ __forceinline__ WarpAxes tf_warp_axes(const WarpTaps &t, float x, float y)
{
    WarpAxes a;
    a.x1 = (float)t.x1 - x; a.x0 = x - (float)t.x0;
    a.y1 = (float)t.y1 - y; a.y0 = y - (float)t.y0;
    return a;
}
// one channel's share of (d L / d x, d L / d y), g = d L / d out of that channel, added to (gx, gy) in channel order
__device__ __forceinline__ void tf_warp_slope(const WarpAxes &a, float Ia, float Ib, float Ic, float Id, float g, float &gx, float &gy)
{
    gx = gx + (a.y1 * (Ic - Ia) + a.y0 * (Id - Ib)) * g;
    gy = gy + (a.x1 * (Ib - Ia) + a.x0 * (Id - Ic)) * g;
}

}  // namespace vstab
