// A refinement level's two hand-written pieces as entry points of their own (tests/test_gpu_refine_level.py): the transposed convolution in
// Winograd F(2x2,2x2) form (vstab_deconv4x4_winograd: input transform, 9-position GEMM, inverse transform -- alone or riding in the flow
// head's launch, as in the forward) and the flow head (vstab_predict_up), plus the Winograd-domain operand packer for arbitrary channel
// counts.  No arithmetic here: argument checks, then the launchers the forward uses.
#include <algorithm>
#include <vector>

#include "api_internal.h"
#include "conv_desc.h"

using namespace vstab;

namespace {
constexpr long long GIB2 = 0x80000000LL;

bool misaligned(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

// the flow head's arguments: what launch_predict_up refuses, and what its kernels' 32-bit indices and vector accesses need
int check_head(const char *who, const float *taps, int ks, long long slab_stride, int B, int h, int w, const float *bias2, const float *prev, int ph,
               int pw, const float *out, const float *up_w, const float *up_b, const float *concat, int oh, int ow, int Cs, int c_off)
{
    if (!taps || !bias2 || !out || !up_w || !up_b || !concat) return fail(nullptr, VSTAB_E_STATE, "%s: NULL buffer", who);
    if (B < 1 || B > 65535 || h < 1 || w < 1 || ks < 1 || oh < 1 || ow < 1 || oh > 2 * h || ow > 2 * w || Cs < 4 || (Cs & 3) || c_off < 0 || (c_off & 3) ||
        c_off + 4 > Cs || (prev && (ph < 1 || pw < 1)))
        return fail(nullptr, VSTAB_E_SHAPE, "%s: needs ks >= 1, oh <= 2 h, ow <= 2 w, Cs %% 4 == 0, c_off %% 4 == 0, c_off + 4 <= Cs", who);
    const long long table = (long long)B * h * w * 32;
    if (slab_stride < 0 || (slab_stride & 1) || (ks > 1 && slab_stride < table))
        return fail(nullptr, VSTAB_E_SHAPE, "%s: slab_stride must be even and at least one table (%lld floats)", who, table);
    if (((long long)(ks - 1) * slab_stride + table) * 4 >= GIB2 || (long long)B * oh * ow * Cs * 4 >= GIB2 ||
        (prev && (long long)B * ph * pw * 8 >= GIB2))
        return fail(nullptr, VSTAB_E_SHAPE, "%s: every tensor must stay below 2 GiB", who);
    if (misaligned(taps, 8) || misaligned(out, 8) || misaligned(prev, 8) || misaligned(concat, 16))
        return fail(nullptr, VSTAB_E_ALIGN, "%s: 8-byte taps / prev / out, 16-byte concat", who);
    return VSTAB_OK;
}

UpflowW upflow(const float *up_w, const float *up_b)
{
    UpflowW W;
    std::memcpy(W.w, up_w, sizeof W.w);
    W.b[0] = up_b[0]; W.b[1] = up_b[1];
    return W;
}

// the Winograd form's shapes: what wdec_applies (flownet_plan.cpp) and the launchers refuse
bool wdec_shape_ok(int B, int Hi, int Wi, int cs_in, int Ho, int Wo, int cs_out, int c_off, int cout, int act, int tile)
{
    if (B < 1 || B > 65535 || Hi < 1 || Wi < 1 || cs_in < 4 || (cs_in & 3) || cout < 1 || ((4 * cout) & 127) || 4 * cout > 2048) return false;
    if ((Ho != 2 * Hi - 1 && Ho != 2 * Hi) || (Wo != 2 * Wi - 1 && Wo != 2 * Wi) || Ho < 1 || Wo < 1) return false;
    if ((cs_out & 3) || c_off < 0 || (c_off & 3) || c_off + cout > cs_out || (act != 0 && act != 1) || (tile != 0 && tile != 1)) return false;
    const WdecGeom g = wdec_geom(Hi, Wi, Ho, Wo);
    const long long planes = (long long)B * 9 * g.NTy * g.NTx;
    return (long long)B * Hi * Wi * cs_in * 4 < GIB2 && (long long)B * Ho * Wo * cs_out * 4 < GIB2 &&
           planes * std::max(cs_in, 4 * cout) * 4 < GIB2 && 9LL * klayout_run(1, 1, cs_in).ktiles() * 4 * cout * 128 < GIB2;
}
}  // namespace

extern "C" long long vstab_host_pack_wdec_shape(const float *W, const double *scale, int cin, int cs_in, int cout, float *wpk, long long cap)
{
    if (!W || !wpk || cin < 1 || cs_in < cin || cout < 1) return fail(nullptr, VSTAB_E_SHAPE, "pack_wdec: bad arguments");
    const long long n = 9LL * klayout_run(1, 1, cs_in).ktiles() * 4 * cout * 32;
    if (cap < n) return fail(nullptr, VSTAB_E_NOMEM, "pack_wdec: need %lld floats", n);
    std::vector<double> ones;
    if (!scale) { ones.assign(cout, 1.0); scale = ones.data(); }
    pack_wdec(W, scale, cin, cs_in, cout, wpk);
    return n;
}

extern "C" size_t vstab_deconv4x4_winograd_workspace_bytes(int B, int Hi, int Wi, int cs_in, int Ho, int Wo, int cout)
{
    if (!wdec_shape_ok(B, Hi, Wi, cs_in, Ho, Wo, cout, 0, cout, 0, 0)) return 0;
    const WdecGeom g = wdec_geom(Hi, Wi, Ho, Wo);
    const size_t planes = (size_t)B * 9 * g.NTy * g.NTx;
    return a256(planes * cs_in * 4) + a256(planes * 4 * cout * 4) + a256((size_t)4 * cout * 4);      // V, M, the GEMM's zero bias
}

extern "C" int vstab_deconv4x4_winograd(const float *x, int B, int Hi, int Wi, int cs_in, const float *wpk, const float *bias, int act, float *out,
                                        int Ho, int Wo, int cs_out, int c_off, int cout, int tile, const vstab_predict_up_args *head,
                                        void *workspace, size_t workspace_bytes, void *stream)
{
    if (!x || !wpk || !bias || !out || !workspace) return fail(nullptr, VSTAB_E_STATE, "deconv4x4_winograd: NULL buffer");
    if (!wdec_shape_ok(B, Hi, Wi, cs_in, Ho, Wo, cs_out, c_off, cout, act, tile))
        return fail(nullptr, VSTAB_E_SHAPE, "deconv4x4_winograd: needs cs_in %% 4 == 0, 4 cout a multiple of 128 up to 2048, Ho in {2 Hi - 1, 2 Hi} "
                                            "(Wo likewise), a 4-aligned output slice, act and tile 0 or 1, < 2 GiB per tensor");
    if (misaligned(x, 16) || misaligned(wpk, 16) || misaligned(bias, 16) || misaligned(out, 16) || misaligned(workspace, 256))
        return fail(nullptr, VSTAB_E_ALIGN, "deconv4x4_winograd: 16-byte tensors, 256-byte workspace");
    if (head)
        if (const int rc = check_head("deconv4x4_winograd: head", head->taps, head->ks, head->slab_stride, B, head->h, head->w, head->bias2, head->prev,
                                      head->ph, head->pw, head->out, head->up_w, head->up_b, head->concat, head->oh, head->ow, head->Cs, head->c_off))
            return rc;
    if (workspace_bytes < vstab_deconv4x4_winograd_workspace_bytes(B, Hi, Wi, cs_in, Ho, Wo, cout))
        return fail(nullptr, VSTAB_E_NOMEM, "deconv4x4_winograd: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const WdecGeom g = wdec_geom(Hi, Wi, Ho, Wo);
    const size_t planes = (size_t)B * 9 * g.NTy * g.NTx;
    char *ws = reinterpret_cast<char *>(workspace);
    float *V = reinterpret_cast<float *>(ws); ws += a256(planes * cs_in * 4);
    float *M = reinterpret_cast<float *>(ws); ws += a256(planes * 4 * cout * 4);
    float *bz = reinterpret_cast<float *>(ws);
    HIP_TRY(nullptr, conv_set_attributes());
    HIP_TRY(nullptr, hipMemsetAsync(bz, 0, (size_t)4 * cout * sizeof(float), st));
    HIP_TRY(nullptr, launch_wdec_input(x, B, Hi, Wi, cs_in, V, g, st));
    ConvParams q = conv_desc_wdec_gemm(B, g, cs_in, cout);
    q.in = V; q.out = M; q.wpk = wpk; q.bias = bz; q.partial = nullptr;
    HIP_TRY(nullptr, launch_conv(q, tile == 0 ? TILE_128x128 : TILE_64x128, true, st));
    if (!head) {
        HIP_TRY(nullptr, launch_wdec_output(M, B, Ho, Wo, cout, bias, act, out, cs_out, c_off, g, st));
        return VSTAB_OK;
    }
    // the inverse transform rides in the flow head's launch (wdec_output_predict_up_kernel), as in the forward
    const WdecOutArgs wo{M, cout / 4, bias, act, out, Ho, Wo, cs_out, c_off, g};
    HIP_TRY(nullptr, launch_predict_up(head->taps, head->ks, head->slab_stride, B, head->h, head->w, head->bias2, head->prev, head->ph, head->pw,
                                       head->out, upflow(head->up_w, head->up_b), head->concat, head->oh, head->ow, head->Cs, head->c_off, st,
                                       nullptr, &wo));
    return VSTAB_OK;
}

extern "C" int vstab_predict_up(const float *taps, int ks, long long slab_stride, int B, int h, int w, const float *bias2, const float *prev, int ph,
                                int pw, float *out, const float *up_w, const float *up_b, float *concat, int oh, int ow, int Cs, int c_off,
                                void *stream)
{
    if (const int rc = check_head("predict_up", taps, ks, slab_stride, B, h, w, bias2, prev, ph, pw, out, up_w, up_b, concat, oh, ow, Cs, c_off))
        return rc;
    HIP_TRY(nullptr, launch_predict_up(taps, ks, slab_stride, B, h, w, bias2, prev, ph, pw, out, upflow(up_w, up_b), concat, oh, ow, Cs, c_off,
                                       (hipStream_t)stream, nullptr, nullptr));
    return VSTAB_OK;
}
