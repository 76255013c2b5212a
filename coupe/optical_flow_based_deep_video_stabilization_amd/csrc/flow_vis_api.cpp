// C ABI of the flow visualisation of flow_vis.py (flow_to_image, main_flownetS_pyramid.py:824-957): argument checks and the
// workspace size.  The kernels are in flow_vis_ops.hip.
#include "api_internal.h"

using namespace vstab;

namespace {

// 1 <= B <= 65535 (a grid dimension), H, W >= 1, fewer than 2^31 pixels in all
bool flow_vis_shape_ok(int B, int H, int W)
{
    return B >= 1 && B <= 65535 && H >= 1 && W >= 1 && (long long)B * H * W < (1LL << 31);
}

}  // namespace

extern "C" size_t vstab_flow_to_image_workspace_bytes(int B, int H, int W)
{
    if (!flow_vis_shape_ok(B, H, W)) return 0;
    return a256((size_t)B * flow_vis_partials(H, W) * sizeof(float));
}

extern "C" int vstab_flow_to_image(const float *flow, int B, int H, int W, const float *maxrad_in, unsigned char *img, unsigned char *anglemap,
                                   float *maxrad_out, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!flow || !img || (!maxrad_in && !workspace)) return fail(nullptr, VSTAB_E_STATE, "flow_to_image: NULL buffer");
    if (!flow_vis_shape_ok(B, H, W))
        return fail(nullptr, VSTAB_E_SHAPE, "flow_to_image: need 1 <= B <= 65535, H, W >= 1 and fewer than 2^31 pixels, got %dx%dx%d", B, H, W);
    if (((uintptr_t)flow) & 7) return fail(nullptr, VSTAB_E_ALIGN, "flow_to_image: flow must be 8-byte aligned");
    if ((((uintptr_t)maxrad_in) | ((uintptr_t)maxrad_out)) & 3) return fail(nullptr, VSTAB_E_ALIGN, "flow_to_image: radii must be 4-byte aligned");
    if (!maxrad_in) {
        if (((uintptr_t)workspace) & 3) return fail(nullptr, VSTAB_E_ALIGN, "flow_to_image: workspace must be 4-byte aligned");
        const size_t need = vstab_flow_to_image_workspace_bytes(B, H, W);
        if (workspace_bytes < need) return fail(nullptr, VSTAB_E_NOMEM, "flow_to_image: workspace %zu < %zu bytes", workspace_bytes, need);
    }
    HIP_TRY(nullptr, launch_flow_to_image(flow, B, H, W, maxrad_in, img, anglemap, maxrad_out, (float *)workspace, (hipStream_t)stream));
    return VSTAB_OK;
}
