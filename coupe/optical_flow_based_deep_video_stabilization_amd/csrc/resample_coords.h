// The index maps of the reference's two resamplers, stated once for the forward kernels (flow_ops.hip), the backward kernels that re-derive
// the forward's indices (train_ops.hip) and the host code that sizes LDS windows with them: the same fp32 operations in the same order.
#pragma once
#include "vstab_internal.h"
#include <math.h>

namespace vstab {
__host__ __device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }      // a ternary: one body for host and device
// legacy TF bilinear (ResizeBilinear, align_corners=False, no half-pixel centres):
// f = i * (in/out) in fp32, lo = floor(f), hi = min(lo+1, in-1), t = f - lo
struct Lerp { int lo, hi; float t; };
__host__ __device__ __forceinline__ Lerp legacy_coord(int o, float scale, int n_in)
{
    const float f = (float)o * scale;
    const float fl = floorf(f);
    Lerp L;
    L.lo = imin((int)fl, n_in - 1);
    L.hi = imin(L.lo + 1, n_in - 1);
    L.t = f - fl;
    return L;
}
__host__ __device__ __forceinline__ float lerp2(float tl, float tr, float bl, float br, float tx, float ty)
{
    const float top = tl + (tr - tl) * tx;
    const float bot = bl + (br - bl) * tx;
    return top + (bot - top) * ty;
}
// nearest neighbour with align_corners=True: src = min((int)roundf(i * (in-1)/(out-1)), in-1)
__host__ __device__ __forceinline__ int nearest_ac(int i, float scale, int n_in) { return imin((int)roundf((float)i * scale), n_in - 1); }

}  // namespace vstab
