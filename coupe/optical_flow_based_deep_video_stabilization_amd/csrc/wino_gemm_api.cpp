// The 16 Winograd-domain GEMMs of a 3x3 stride-1 stage as an entry point of their own (vstab_wino_domain_gemm: the tiled launch and the
// streams of positions on ONE packed operand, tests/test_gpu_wino_gemm_stream.py) and the host-only views of the stream form's rule and of
// the operand packing.  No arithmetic here: argument checks, then the launchers the forward uses.
#include <vector>

#include "api_internal.h"
#include "conv_desc.h"

using namespace vstab;

namespace {
// every tensor of the call below 2 GiB (the kernels' buffer descriptors and 32-bit offsets), channels whole K-tiles / column tiles
bool gemm_shape_ok(int B, int T, int cin, int cout)
{
    if (B < 1 || T < 1 || cin < 32 || (cin & 31) || cout < 64 || (cout & 63)) return false;
    const long long rows = (long long)B * 16 * T;
    return rows * cin * 4 < 0x80000000LL && rows * cout * 4 < 0x80000000LL && 16LL * cin * cout * 4 < 0x80000000LL;
}
}  // namespace

extern "C" int vstab_host_wino_stream_positions(int B, int T, int cin, int cout)
{
    return wino_gemm_stream_positions(B, T, cin, cout);
}

extern "C" long long vstab_host_pack_winograd(const float *W, const double *scale, int cin, int cout, float *wpk, long long cap)
{
    if (!W || !wpk || cin < 1 || cout < 1) return fail(nullptr, VSTAB_E_SHAPE, "pack_winograd: bad arguments");
    const long long n = 16LL * klayout_run(1, 1, cin).ktiles() * cout * 32;
    if (cap < n) return fail(nullptr, VSTAB_E_NOMEM, "pack_winograd: need %lld floats", n);
    std::vector<double> ones;
    if (!scale) { ones.assign(cout, 1.0); scale = ones.data(); }
    pack_winograd(W, scale, cin, cout, cout, wpk);
    return n;
}

extern "C" size_t vstab_wino_domain_gemm_workspace_bytes(int B, int T, int cin, int cout)
{
    if (!gemm_shape_ok(B, T, cin, cout)) return 0;
    return a256((size_t)16 * cin * cout * 4) + a256((size_t)cout * 4);         // the packed operand, the tiled launch's zero bias
}

extern "C" int vstab_wino_domain_gemm(const float *V, const float *U, float *M, int B, int T, int cin, int cout, int form, void *workspace,
                                      size_t workspace_bytes, void *stream)
{
    if (!V || !U || !M || !workspace) return fail(nullptr, VSTAB_E_STATE, "wino_domain_gemm: NULL buffer");
    if (!gemm_shape_ok(B, T, cin, cout) || (form != 0 && form != 1))
        return fail(nullptr, VSTAB_E_SHAPE, "wino_domain_gemm: needs cin %% 32 == 0, cout %% 64 == 0, < 2 GiB per tensor, form 0 or 1");
    if (((reinterpret_cast<uintptr_t>(V) | reinterpret_cast<uintptr_t>(U) | reinterpret_cast<uintptr_t>(M)) & 15) ||
        (reinterpret_cast<uintptr_t>(workspace) & 255))
        return fail(nullptr, VSTAB_E_ALIGN, "wino_domain_gemm: 16-byte tensors, 256-byte workspace");
    const int P = form == 1 ? wino_gemm_stream_positions(B, T, cin, cout) : 0;
    if (form == 1 && P == 0) return fail(nullptr, VSTAB_E_SHAPE, "wino_domain_gemm: the stream form does not take B=%d T=%d %d -> %d", B, T, cin, cout);
    if (workspace_bytes < vstab_wino_domain_gemm_workspace_bytes(B, T, cin, cout))
        return fail(nullptr, VSTAB_E_NOMEM, "wino_domain_gemm: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    char *ws = reinterpret_cast<char *>(workspace);
    float *wpk = reinterpret_cast<float *>(ws); ws += a256((size_t)16 * cin * cout * 4);
    float *bz = reinterpret_cast<float *>(ws);
    HIP_TRY(nullptr, launch_pack_blocked(U, cin, cout, cout, 16, wpk, st));      // 16 x [cin][cout] -> 16 x [cin/32][cout][32]
    if (form == 1) {
        HIP_TRY(nullptr, wino_gemm_stream_set_attributes());
        HIP_TRY(nullptr, launch_wino_gemm_stream(V, wpk, M, B, T, cin, cout, P, st, nullptr, nullptr));
        return VSTAB_OK;
    }
    HIP_TRY(nullptr, conv_set_attributes());
    HIP_TRY(nullptr, hipMemsetAsync(bz, 0, (size_t)cout * sizeof(float), st));
    ConvParams p = conv_desc_wino_gemm(B, 2, 2 * T, cin, cout);                 // the forward's descriptor for planes of 1 x T tiles
    p.in = V; p.out = M; p.wpk = wpk; p.bias = bz; p.partial = nullptr;
    HIP_TRY(nullptr, launch_conv(p, TILE_128x64, true, st));
    return VSTAB_OK;
}

extern "C" int vstab_wino_gemm_stream_launch(const float *V, const float *wpk, float *M, int B, int T, int cin, int cout, int P, void *stream)
{
    if (!V || !wpk || !M) return fail(nullptr, VSTAB_E_STATE, "wino_gemm_stream_launch: NULL buffer");
    if ((reinterpret_cast<uintptr_t>(V) | reinterpret_cast<uintptr_t>(wpk) | reinterpret_cast<uintptr_t>(M)) & 15)
        return fail(nullptr, VSTAB_E_ALIGN, "wino_gemm_stream_launch: 16-byte tensors");
    HIP_TRY(nullptr, wino_gemm_stream_set_attributes());
    const hipError_t e = launch_wino_gemm_stream(V, wpk, M, B, T, cin, cout, P, (hipStream_t)stream, nullptr, nullptr);
    if (e == hipErrorInvalidValue) return fail(nullptr, VSTAB_E_SHAPE, "wino_gemm_stream_launch: the launcher refuses B=%d T=%d %d -> %d with P=%d", B, T, cin, cout, P);
    HIP_TRY(nullptr, e);
    return VSTAB_OK;
}
