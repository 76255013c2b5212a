// Launchers of csrc/theta_ops.hip (the theta regressors' blocks; the contract of each is its entry point's in include/vstab.h) and the
// dense layer's slab plan.  The launchers check nothing: theta_api.cpp does.
#pragma once
#include <hip/hip_runtime.h>

namespace vstab {

// vstab_dense_forward's cut of K: `rows` rows of W per slab (a multiple of 4), `slabs` of them, `tiles` column tiles of `vec` * 64
// columns (vec = 4 when a row of W can be read 16 bytes at a time, else 1).  A function of K and N alone.
struct DensePlan {
    int rows, slabs, tiles, vec;
};
DensePlan dense_plan(int K, int N);

hipError_t launch_pad_symmetric(const float *x, int B, int H, int W, int C, int p, float *y, int cs_y, hipStream_t stream);
hipError_t launch_bn_lrelu_slope_inference(float *zy, long long rows, int cs, int c_off, int C, const float *beta, const float *mov_mean,
                                           const float *mov_var, float eps, float slope, int twice, hipStream_t stream);
hipError_t launch_bn_lrelu_slope_pool_inference(const float *z, int B, int H, int W, int C, const float *beta, const float *mov_mean,
                                                const float *mov_var, float eps, float slope, int twice, float *out, hipStream_t stream);
hipError_t launch_dense_forward(const float *x, int B, int K, int N, const float *W, const float *b, int act, float slope, const float *scale,
                                const float *shift, float *y, float *partial, hipStream_t stream);

}  // namespace vstab
