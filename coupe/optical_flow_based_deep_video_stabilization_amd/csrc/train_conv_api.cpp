// C ABI of the training step's convolutions: filter / bias gradient, input gradient, the forward on raw weights, the
// row-window first layer, both Winograd forms.  Each keeps a per-geometry plan for the life of the process (plan_cache.h); what a plan
// decides is a pure function of the geometry, and only its index table lives on the device.
#include <algorithm>
#include <array>
#include <cstdint>
#include <vector>

#include "../../../include/vstab.h"
#include "api_internal.h"
#include "conv_desc.h"
#include "plan_cache.h"
#include "vstab_internal.h"

using namespace vstab;

namespace {
// ------------------------------------------------------------------------- shape rules
// The kernels address a tensor through a buffer descriptor with 32-bit byte offsets.
bool below_2gib(int B, int H, int W, int cs) { return (long long)B * H * W * cs * 4 < 0x80000000LL; }

// Ho x Wo is the symmetric-pad output size of a k x k / stride / pad conv over Hi x Wi or -- extra -- one more row and / or column:
// TF's SAME conv of an odd size pads one more at the end, and a transposed conv with a cropped output_shape (model.py:850: 23 <- 12)
// is exactly that case.  The windows that stick out of the image lose those taps (range checks: they read zero).
bool out_size_ok(int Hi, int Wi, int k, int stride, int pad, int Ho, int Wo, bool extra)
{
    const int dh = Ho - ((Hi + 2 * pad - k) / stride + 1), dw = Wo - ((Wi + 2 * pad - k) / stride + 1);
    return dh >= 0 && dw >= 0 && dh <= (extra ? 1 : 0) && dw <= (extra ? 1 : 0);
}

// ------------------------------------------------------------------------- filter gradient (wgrad_mfma.hip)
// The weight-gradient kernel's per-output-pixel table depends on the geometry only: built once per (device, geometry) and kept
// for the life of the process (16 B per output pixel; a training step used to rebuild 23 of them).
const int4 *wgrad_pixel_table(int B, int Hi, int Wi, int cs_x, int Ho, int Wo, int stride, int pad, hipStream_t st)
{
    static PlanCache<int4 *, 8> cache(true);
    int4 *t = nullptr;
    cache.get({B, Hi, Wi, cs_x, Ho, Wo, stride, pad}, t, [&](int4 *&d) {
        if (hipMalloc(reinterpret_cast<void **>(&d), (size_t)B * Ho * Wo * sizeof(int4)) != hipSuccess) return false;
        // built on the caller's stream and completed before anyone (on any stream) can be handed the cached pointer
        if (launch_wgrad_pixel_table(B, Hi, Wi, cs_x, Ho, Wo, stride, pad, d, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess) return true;
        (void)hipFree(d);
        return false;
    });
    return t;
}

// How a filter gradient with `cout` columns is launched: as one launch, or -- 128 k + a few columns (the decoder's concat inputs:
// 1026 / 770 / 386 channels + padding) -- as its 128-wide part plus a narrow tail, instead of a whole 128-column tile row for the tail.
struct WgradSplit { int n_main, n_tail, ks_main, ks_tail; size_t slab_floats; };
WgradSplit wgrad_split(int M, int cout, int K)
{
    WgradSplit s{};
    WgradParams p{};
    p.M = M; p.K = K;
    s.n_main = cout / 128 * 128; s.n_tail = cout - s.n_main;
    if (!(s.n_main >= 128 && s.n_tail > 0 && s.n_tail <= 32)) { s.n_main = cout; s.n_tail = 0; }
    p.Cout = s.n_main; s.ks_main = wgrad_choose_split(p);
    s.slab_floats = s.ks_main > 1 ? (size_t)s.ks_main * M * s.n_main : 0;
    if (s.n_tail) {
        p.Cout = s.n_tail; s.ks_tail = wgrad_choose_split(p);
        s.slab_floats = std::max(s.slab_floats, s.ks_tail > 1 ? (size_t)s.ks_tail * M * s.n_tail : 0);      // the launches run one after the other
    }
    return s;
}

// workspace of vstab_conv_wgrad: the split-K slabs at 0, then the bias gradient's column-sum scratch
struct WgradWs { size_t colsum, total; };
WgradWs wgrad_ws(const WgradSplit &s, long long K, int cout)
{
    WgradWs w{};
    w.colsum = a256(s.slab_floats * sizeof(float));
    w.total = w.colsum + (size_t)column_sum_chunks(K, cout) * cout * sizeof(float) + 256;
    return w;
}

// the 16-plane batched launch of the Winograd form: M = cin rows, a reduction over T = B*TH*TW tiles
bool wino_wgrad_shape(int B, int H, int W, int cin, int cout, WgradParams &p, int &TH, int &TW)
{
    if (B < 1 || H < 1 || W < 1 || cin < 4 || cout < 4 || (cin & 3) || (cout & 3)) return false;
    TH = (H + 1) / 2; TW = (W + 1) / 2;
    const long long T = (long long)B * TH * TW;
    if (T * 16 * std::max(cin, cout) * 4 >= 0x80000000LL || T * std::max(cin, cout) * 4 >= 0x80000000LL) return false;
    p = WgradParams{};
    p.Hi = (int)T; p.Wi = 1; p.Cs_x = cin; p.cx_off = 0; p.Cin = cin; p.KH = 1; p.KW = 1;
    p.Cs_g = cout; p.cg_off = 0; p.Cout = cout; p.M = cin; p.K = (int)T;
    p.nbatch = 16;
    p.ksplit = wgrad_choose_split(p);
    return true;
}

// workspace of vstab_conv3x3_winograd_wgrad: V [16][T][cin], dM [16][T][cout], dU [16][cin][cout], the split-K slabs
struct WinoWgradWs { size_t dM, dU, partial, total; };
WinoWgradWs wino_wgrad_ws(size_t T, int cin, int cout, int ksplit)
{
    WinoWgradWs w{};
    w.dM = a256(T * 16 * cin * 4);
    w.dU = w.dM + a256(T * 16 * cout * 4);
    w.partial = w.dU + a256((size_t)16 * cin * cout * 4);
    w.total = w.partial + a256(ksplit > 1 ? (size_t)16 * ksplit * cin * cout * 4 : 0) + 256;
    return w;
}
}  // namespace

// Host-only view of the two rules above (no HIP call): out4 = {n_main, n_tail, ks_main, ks_tail} of the launches vstab_conv_wgrad makes of a
// reduction over K pixels into M x cout (nbatch 0 or 1), or -- nbatch 16 -- {cout, 0, ksplit, 0} of the batched launch that
// vstab_conv3x3_winograd_wgrad makes for M = cin input channels and K = B*TH*TW tiles.
extern "C" int vstab_host_wgrad_split(int M, int cout, int K, int nbatch, int *out4)
{
    if (!out4 || M < 1 || cout < 1 || K < 1 || !(nbatch == 0 || nbatch == 1 || nbatch == 16)) return VSTAB_E_SHAPE;
    if (nbatch == 16) {
        WgradParams p; int TH, TW;
        if (!wino_wgrad_shape(K, 1, 1, M, cout, p, TH, TW)) return VSTAB_E_SHAPE;              // K samples of one tile each: T = K
        out4[0] = p.Cout; out4[1] = 0; out4[2] = p.ksplit; out4[3] = 0;
        return VSTAB_OK;
    }
    const WgradSplit s = wgrad_split(M, cout, K);
    out4[0] = s.n_main; out4[1] = s.n_tail; out4[2] = s.ks_main; out4[3] = s.ks_tail;
    return VSTAB_OK;
}

extern "C" size_t vstab_conv_wgrad_workspace_bytes(int B, int Ho, int Wo, int k, int cin, int cout)
{
    if (B < 1 || Ho < 1 || Wo < 1 || k < 1 || cin < 1 || cout < 1) return 0;
    return wgrad_ws(wgrad_split(k * k * cin, cout, B * Ho * Wo), (long long)B * Ho * Wo, cout).total;
}

extern "C" int vstab_conv_wgrad(const float *x, int B, int Hi, int Wi, int cs_x, int cx_off, int cin, const float *gout, int Ho,
                                int Wo, int cs_g, int cg_off, int cout, int k, int stride, int pad, float *dW, float *db,
                                int accumulate, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!x || !gout || !dW || !workspace) return fail(nullptr, VSTAB_E_STATE, "conv_wgrad: NULL buffer");
    if (B < 1 || Hi < 1 || Wi < 1 || Ho < 1 || Wo < 1 || k < 1 || k > 7 || stride < 1 || pad < 0 || cin < 1 || cout < 1 ||
        cx_off < 0 || cg_off < 0 || cx_off + cin > cs_x || cg_off + cout > cs_g)
        return fail(nullptr, VSTAB_E_SHAPE, "conv_wgrad: bad shape");
    if (!out_size_ok(Hi, Wi, k, stride, pad, Ho, Wo, true))
        return fail(nullptr, VSTAB_E_SHAPE, "conv_wgrad: %dx%d input, k %d stride %d pad %d does not match a %dx%d output", Hi, Wi, k,
                    stride, pad, Ho, Wo);
    if ((cin & 3) || (cs_x & 3) || (cx_off & 3) || (cs_g & 3) || (cg_off & 3))
        return fail(nullptr, VSTAB_E_ALIGN, "conv_wgrad: channel counts, strides and offsets must be multiples of 4");
    if (!below_2gib(B, Hi, Wi, cs_x) || !below_2gib(B, Ho, Wo, cs_g))
        return fail(nullptr, VSTAB_E_SHAPE, "conv_wgrad: tensors must stay below 2 GiB");
    if ((reinterpret_cast<uintptr_t>(x) & 15) || (reinterpret_cast<uintptr_t>(gout) & 15) || (reinterpret_cast<uintptr_t>(workspace) & 255))
        return fail(nullptr, VSTAB_E_ALIGN, "conv_wgrad: x / gout must be 16-byte, workspace 256-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    WgradParams p{};
    p.x = x; p.g = gout; p.dW = dW;
    p.x_bytes = (unsigned)((long long)B * Hi * Wi * cs_x * 4); p.g_bytes = (unsigned)((long long)B * Ho * Wo * cs_g * 4);
    p.Hi = Hi; p.Wi = Wi; p.Cs_x = cs_x; p.cx_off = cx_off; p.Cin = cin; p.KH = k; p.KW = k;
    p.Cs_g = cs_g; p.cg_off = cg_off; p.Cout = cout; p.M = k * k * cin; p.K = B * Ho * Wo;
    p.accumulate = accumulate ? 1 : 0;
    const WgradSplit sp = wgrad_split(p.M, cout, p.K);
    const WgradWs w = wgrad_ws(sp, p.K, cout);
    if (workspace_bytes < w.total) return fail(nullptr, VSTAB_E_NOMEM, "conv_wgrad: workspace %zu < %zu bytes", workspace_bytes, w.total);
    p.ptab = wgrad_pixel_table(B, Hi, Wi, cs_x, Ho, Wo, stride, pad, st);
    if (!p.ptab) return fail(nullptr, VSTAB_E_NOMEM, "conv_wgrad: cannot build the pixel table");
    p.partial = reinterpret_cast<float *>(workspace);
    p.Cout = sp.n_main; p.ldw = cout; p.col0 = 0; p.ksplit = sp.ks_main;
    HIP_TRY(nullptr, launch_wgrad(p, st));
    if (sp.n_tail) {
        p.Cout = sp.n_tail; p.cg_off = cg_off + sp.n_main; p.col0 = sp.n_main; p.ksplit = sp.ks_tail;
        HIP_TRY(nullptr, launch_wgrad(p, st));
    }
    if (db) {
        float *scratch = reinterpret_cast<float *>(reinterpret_cast<char *>(workspace) + w.colsum);
        HIP_TRY(nullptr, launch_column_sum(gout, (long long)p.K, cs_g, cg_off, cout, db, accumulate ? 1 : 0, scratch, st));
    }
    return VSTAB_OK;
}

// ------------------------------------------------------------------------- convolutions in GEMM form on raw weights
namespace {
// a zero vector every bias-less GEMM can point at (instead of a memset in front of each launch); 8192 floats per device, never freed
const float *zero_bias()
{
    static PlanCache<float *, 0> cache(true);
    float *z = nullptr;
    cache.get({}, z, [](float *&p) {
        if (hipMalloc(reinterpret_cast<void **>(&p), 8192 * sizeof(float)) != hipSuccess) return false;
        if (hipMemset(p, 0, 8192 * sizeof(float)) == hipSuccess) return true;
        (void)hipFree(p);
        return false;
    });
    return z;
}

// Does a gather table read its source contiguously along the output column?  Sampled: for logical k, the entries of columns n and n + 1
// (both live) differ by one.  Rows of the packed operand are [K-tile][Npad][32] with the 16-byte chunks of column n swizzled by (n >> 1) & 7.
bool table_is_n_fast(const std::vector<int32_t> &tbl, int npad)
{
    long long hit = 0, seen = 0;
    const size_t rows = tbl.size() / 32;
    for (size_t r = 0; r + 1 < rows && seen < 4096; r += 7) {
        const int n = (int)(r % npad);
        if (n + 1 >= npad) continue;
        for (int k = 0; k < 32; k += 5) {
            const int32_t a = tbl[r * 32 + swz32(n, k)], b = tbl[(r + 1) * 32 + swz32(n + 1, k)];
            if (a > 0 && b > 0) { ++seen; hit += (b == a + 1); }
        }
    }
    return seen >= 16 && hit * 10 >= seen * 9;
}

// A convolution as implicit GEMMs whose operand is gathered on the device, every call, from the caller's raw weights (the weights of a
// training run change every step): the forward, and the input gradient = a convolution over gout with the channel roles swapped.
struct GemmConvPlan {
    ConvParams p;
    ConvTile tile;
    bool vec4;
    size_t packed_floats;       // all phases
    int32_t *tbl;               // device index table, owned by the cache (NULL when `blocked_K`)
    bool tbl_nfast;             // the table's sources run contiguously along the output column: the LDS-transposing replay (train_ops.hip)
    int blocked_K;              // > 0: the operand is a plain [K][N] matrix -> launch_pack_blocked instead of the table
    // odd-k stride-2 input gradients: the four output-parity phases have DIFFERENT tap counts ((k+1)/2 or (k-1)/2 per axis), so each
    // is its own launch with exactly its taps instead of one 4-phase launch padded to ceil(k/2)^2 (44 % / 31 % of the MACs of a
    // 3x3 / 5x5 layer were zero taps).  nsub == 0: the single launch `p` is the whole plan.
    int nsub;
    ConvParams sp[4];
    ConvTile stile[4];
    size_t soff[4];             // float offset of each phase's operand inside the packed buffer / the table
    size_t part_floats;         // split-K slab space (max over the launches)
};

// The input gradient's plan and its gather table (the host packer's gather, recorded once).  No HIP call.  gout is read from its first
// used channel: cs_g stays the pixel stride, the caller moves the pointer by cg_off.
bool plan_dgrad(int B, int Ho, int Wo, int cs_g, int cout, int k, int stride, int pad, int Hi, int Wi, int cs_x, int cx_off, int cin,
                int accumulate, GemmConvPlan &d, std::vector<int32_t> &tbl)
{
    ConvParams &p = d.p;
    const int act = accumulate ? 3 : 0;
    if (stride == 1) {
        // conv over gout with pad k-1-pad, flipped kernel, channel roles swapped
        if (!fill_plain_conv(p, d.tile, d.vec4, B, Ho, Wo, cout, cs_g, k, 1, k - 1 - pad, cin, cs_x, cx_off, act)) return false;
        if (p.Ho != Hi || p.Wo != Wi || !d.vec4) return false;
        const KLayout L{p.KH, p.NSEG, p.SEG, p.SEGP, p.SEG_STRIDE};
        d.packed_floats = (size_t)L.ktiles() * p.Npad * 32;
        tbl.resize(d.packed_floats);
        pack_index_dgrad_s1(k, cin, cout, cs_g, L, p.Npad, tbl.data());
    } else if (k & 1) {
        // one launch per output-parity phase, each with exactly its taps: row taps ky = t0y + 2u (u < nty), input row j + c - u
        if (cs_g & 3) return false;
        const ConvTile base = default_tile(cin);
        const int BN = tile_cols(base), npad = padded_cols(cin, base);
        d.vec4 = true;
        d.packed_floats = 0;
        for (int py = 0; py < 2; ++py)
            for (int px = 0; px < 2; ++px) {
                const int t0y = (py + pad) & 1, t0x = (px + pad) & 1;
                const int nty = (k - t0y + 1) / 2, ntx = (k - t0x + 1) / 2;
                const int Hg = (Hi - py + 1) / 2, Wg = (Wi - px + 1) / 2;
                if (Hg < 1 || Wg < 1 || nty < 1 || ntx < 1) continue;
                ConvParams &q = d.sp[d.nsub];
                q = conv_desc_phase(B, Ho, Wo, cout, cs_g, nty, ntx, 1,
                                    ConvGrid{Hg, Wg, (py + pad - t0y) / 2 - nty + 1, (px + pad - t0x) / 2 - ntx + 1, 2, py, px}, Hi, Wi, cin, npad,
                                    cs_x, cx_off, act);
                if (q.SEG & 3) return false;
                const KLayout L{q.KH, q.NSEG, q.SEG, q.SEGP, q.SEG_STRIDE};
                d.stile[d.nsub] = choose_tile_split(q, base, true);
                d.soff[d.nsub] = d.packed_floats;
                const size_t pf = (size_t)L.ktiles() * npad * 32;
                tbl.resize(d.packed_floats + pf);
                // row tap tt <-> ky = t0y + 2 (nty-1-tt): increasing input row; GEMM columns n = ci, reduction channel = co
                pack_index_phase(k, cin, cout, cs_g, L, npad, t0y, nty, t0x, ntx, tbl.data() + d.packed_floats);
                d.packed_floats += pf;
                if (q.ksplit > 1) d.part_floats = std::max(d.part_floats, (size_t)q.ksplit * q.Mmax * q.Npad);
                ++d.nsub;
            }
        if (d.nsub == 0) return false;
        long long tiles_all = 0;
        for (int s = 0; s < d.nsub; ++s) tiles_all += (long long)((d.sp[s].ph[0].M + 127) / 128) * (npad / BN);
        if (tiles_all <= 256) {
            // Small layers: ONE launch in which every phase carries its own K layout (ConvPhase::KH ...), split-K sized for the four
            // together -- instead of four launches that each fill a fraction of the chip (conv6 at B=8 512x512: 112 -> 85 us; the
            // whole B=1 step 3.45 -> 3.37 ms).  Large layers stay one launch per phase: merged they were SLOWER (conv3 523 -> 585 us,
            // conv2 557 -> 633 us): a launch that works on one phase keeps a quarter of the filter hot in L2.
            p = d.sp[0];
            p.nphase = d.nsub;
            p.Mmax = 0;
            unsigned wmax = 0;
            long long tiles = 0;
            int kt_min = 1 << 30;
            for (int s = 0; s < d.nsub; ++s) {
                const ConvParams &q = d.sp[s];
                ConvPhase &ph = p.ph[s];
                ph = q.ph[0];
                ph.w_off = (long long)d.soff[s];
                ph.KH = q.KH; ph.NSEG = q.NSEG; ph.SEG = q.SEG; ph.SEGP = q.SEGP; ph.SEG_STRIDE = q.SEG_STRIDE;
                p.Mmax = std::max(p.Mmax, ph.M);
                wmax = std::max(wmax, q.w_bytes);
                tiles += (long long)((ph.M + 127) / 128) * (npad / BN);
                kt_min = std::min(kt_min, q.KH * q.NSEG * (q.SEGP / 32));
            }
            p.w_bytes = wmax;
            int ks = (int)(512 / std::max<long long>(tiles, 1));                  // two co-resident workgroups per CU
            ks = std::max(1, std::min(ks, std::max(1, kt_min / 4)));
            p.ksplit = ks;
            d.tile = base;
            d.nsub = 0;
        } else {
            d.p = d.sp[0];
            d.tile = d.stile[0];
        }
    } else {
        // four output-parity phases of ceil(k/2)^2 taps; parity b's first tap is input row j + (b + pad) / 2 - kt2 + 1
        const int kt2 = (k + 1) / 2, off[2] = {pad / 2 - kt2 + 1, (1 + pad) / 2 - kt2 + 1};
        d.tile = default_tile(cin);
        p = conv_desc_parity4(B, Ho, Wo, cout, cs_g, kt2, off, Hi, Wi, cin, padded_cols(cin), cs_x, cx_off, act);
        const KLayout L{p.KH, p.NSEG, p.SEG, p.SEGP, p.SEG_STRIDE};
        const size_t phase_floats = (size_t)L.ktiles() * p.Npad * 32;
        d.vec4 = true;
        if ((cs_g & 3) || (p.SEG & 3)) return false;
        d.tile = choose_tile_split(p, d.tile, true);
        d.packed_floats = 4 * phase_floats;
        tbl.resize(d.packed_floats);
        pack_index_dgrad_s2(k, pad, cin, cout, cs_g, L, p.Npad, tbl.data());
    }
    if (d.nsub == 0 && d.p.ksplit > 1) d.part_floats = (size_t)d.p.nphase * d.p.ksplit * d.p.Mmax * d.p.Npad;
    return true;
}

// The forward's plan; its gather table stays empty when the operand is a plain matrix (blocked_K).  No HIP call.  Ho = Wo = 0: the
// symmetric-pad output size.
bool plan_forward(int B, int Hi, int Wi, int cs_x, int cin, int k, int stride, int pad, int cout, int cs_y, int cy_off, int act, int Ho, int Wo,
                  GemmConvPlan &d, std::vector<int32_t> &tbl)
{
    if (!fill_plain_conv(d.p, d.tile, d.vec4, B, Hi, Wi, cin, cs_x, k, stride, pad, cout, cs_y, cy_off, act)) return false;
    if (Ho > 0 && Wo > 0 && (Ho != d.p.Ho || Wo != d.p.Wo)) {
        if (!out_size_ok(Hi, Wi, k, stride, pad, Ho, Wo, true) || !below_2gib(B, Ho, Wo, cs_y)) return false;
        d.p.Ho = Ho; d.p.Wo = Wo;
        d.p.ph[0].Hg = Ho; d.p.ph[0].Wg = Wo; d.p.ph[0].M = B * Ho * Wo; d.p.Mmax = d.p.ph[0].M;
        d.tile = choose_tile_split(d.p, default_tile(cout), d.vec4);
    }
    const KLayout L{d.p.KH, d.p.NSEG, d.p.SEG, d.p.SEGP, d.p.SEG_STRIDE};
    d.packed_floats = (size_t)L.ktiles() * d.p.Npad * 32;
    if (d.p.ksplit > 1) d.part_floats = (size_t)d.p.nphase * d.p.ksplit * d.p.Mmax * d.p.Npad;
    if (L.NSEG == 1 && L.SEG == L.SEGP && cs_x == cin && (cout & 3) == 0 && (d.p.Npad & 63) == 0) {
        d.blocked_K = L.KH * L.SEG;              // HWIO with its first three axes flattened IS the [K][N] matrix
    } else {
        tbl.resize(d.packed_floats);
        pack_index_conv(k, k, cin, cs_x, cout, d.p.Npad, L, tbl.data());
        d.tbl_nfast = table_is_n_fast(tbl, d.p.Npad);
    }
    return true;
}

// the cached, device-resident forms: the plan of its geometry with its table in the current device's memory
bool dgrad_plan(int B, int Ho, int Wo, int cs_g, int cout, int k, int stride, int pad, int Hi, int Wi, int cs_x, int cx_off, int cin,
                int accumulate, GemmConvPlan &out)
{
    static PlanCache<GemmConvPlan, 14> cache(true);
    return cache.get({B, Ho, Wo, cs_g, cout, k, stride, pad, Hi, Wi, cs_x, cx_off, cin, accumulate}, out, [&](GemmConvPlan &d) {
        std::vector<int32_t> tbl;
        return plan_dgrad(B, Ho, Wo, cs_g, cout, k, stride, pad, Hi, Wi, cs_x, cx_off, cin, accumulate, d, tbl) && (d.tbl = upload_table(tbl));
    });
}

bool fwd_plan(int B, int Hi, int Wi, int cs_x, int cin, int k, int stride, int pad, int cout, int cs_y, int cy_off, int act, int Ho, int Wo,
              GemmConvPlan &out)
{
    static PlanCache<GemmConvPlan, 14> cache(true);
    return cache.get({B, Hi, Wi, cs_x, cin, k, stride, pad, cout, cs_y, cy_off, act, Ho, Wo}, out, [&](GemmConvPlan &d) {
        std::vector<int32_t> tbl;
        return plan_forward(B, Hi, Wi, cs_x, cin, k, stride, pad, cout, cs_y, cy_off, act, Ho, Wo, d, tbl) &&
               (d.blocked_K || (d.tbl = upload_table(tbl)));
    });
}

// workspace of a plan: the packed operand at 0, a padded bias vector, the split-K slabs
struct GemmConvWs { size_t bias, part, total; };
GemmConvWs gemm_conv_ws(const GemmConvPlan &d)
{
    GemmConvWs w{};
    w.bias = a256(d.packed_floats * sizeof(float));
    w.part = w.bias + a256((size_t)d.p.Npad * sizeof(float));
    w.total = w.part + a256(d.part_floats * sizeof(float)) + 256;
    return w;
}

// Runs a plan on the caller's raw weights W: stages the operand, routes the bias, launches.  `in` is the first channel the GEMM
// reads, in_bytes what its tensor holds from there on.
int run_gemm_conv(const char *who, const GemmConvPlan &d, const float *in, unsigned in_bytes, const float *W, const float *bias_in, float *out,
                  void *workspace, size_t workspace_bytes, hipStream_t st)
{
    const GemmConvWs w = gemm_conv_ws(d);
    if (workspace_bytes < w.total) return fail(nullptr, VSTAB_E_NOMEM, "%s: workspace %zu < %zu bytes", who, workspace_bytes, w.total);
    HIP_TRY(nullptr, conv_set_attributes());
    char *ws = reinterpret_cast<char *>(workspace);
    float *wpk = reinterpret_cast<float *>(ws);
    float *bias = reinterpret_cast<float *>(ws + w.bias);
    if (d.blocked_K) HIP_TRY(nullptr, launch_pack_blocked(W, d.blocked_K, d.p.N, d.p.Npad, 1, wpk, st));
    else HIP_TRY(nullptr, launch_pack_apply(W, d.tbl, (long long)d.packed_floats, wpk, st, d.tbl_nfast));
    // the bias vector the kernel reads has Npad entries: a shared zero vector when there is none, the caller's own when it is
    // already that long, a padded copy otherwise
    if (!bias_in && d.p.Npad <= 8192 && zero_bias()) bias = const_cast<float *>(zero_bias());
    else if (bias_in && d.p.N == d.p.Npad) bias = const_cast<float *>(bias_in);
    else {
        HIP_TRY(nullptr, hipMemsetAsync(bias, 0, (size_t)d.p.Npad * sizeof(float), st));
        if (bias_in) HIP_TRY(nullptr, hipMemcpyAsync(bias, bias_in, (size_t)d.p.N * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    const int nl = d.nsub ? d.nsub : 1;
    for (int s = 0; s < nl; ++s) {
        ConvParams p = d.nsub ? d.sp[s] : d.p;
        p.in = in; p.in_bytes = in_bytes;
        p.wpk = wpk + (d.nsub ? d.soff[s] : 0); p.bias = bias; p.out = out;
        p.partial = reinterpret_cast<float *>(ws + w.part);
        HIP_TRY(nullptr, launch_conv(p, d.nsub ? d.stile[s] : d.tile, d.vec4, st));
    }
    return VSTAB_OK;
}

// the refusals of vstab_conv_dgrad that the geometry alone decides, in its order: VSTAB_OK or what fail() returned
int dgrad_geometry_check(int B, int Ho, int Wo, int cs_g, int cg_off, int cout, int k, int stride, int pad, int Hi, int Wi, int cs_x, int cx_off,
                         int cin)
{
    if (B < 1 || Ho < 1 || Wo < 1 || Hi < 1 || Wi < 1 || k < 1 || k > 7 || (stride != 1 && stride != 2) || pad < 0 || pad > k - 1 ||
        cin < 1 || cout < 1 || cg_off < 0 || cx_off < 0 || cg_off + cout > cs_g || cx_off + cin > cs_x)
        return fail(nullptr, VSTAB_E_SHAPE, "conv_dgrad: bad shape (stride must be 1 or 2)");
    // gout may have one more row / column than a symmetric-pad conv of dx's size would give; at stride 1 it may not
    if (!out_size_ok(Hi, Wi, k, stride, pad, Ho, Wo, stride != 1))
        return fail(nullptr, VSTAB_E_SHAPE, "conv_dgrad: %dx%d input, k %d stride %d pad %d does not match a %dx%d output", Hi, Wi, k,
                    stride, pad, Ho, Wo);
    if ((cin & 3) || (cout & 3) || (cs_x & 3) || (cx_off & 3) || (cs_g & 3) || (cg_off & 3))
        return fail(nullptr, VSTAB_E_ALIGN, "conv_dgrad: channel counts, strides and offsets must be multiples of 4");
    if (!below_2gib(B, Hi, Wi, cs_x) || !below_2gib(B, Ho, Wo, cs_g))
        return fail(nullptr, VSTAB_E_SHAPE, "conv_dgrad: tensors must stay below 2 GiB");
    return VSTAB_OK;
}

bool forward_shape_ok(int B, int Hi, int Wi, int cs_x, int cx_off, int cin, int k, int stride, int pad, int cs_y, int cy_off, int cout, int act)
{
    return !(B < 1 || Hi < 1 || Wi < 1 || k < 1 || k > 7 || stride < 1 || pad < 0 || cin < 1 || cout < 1 || cx_off < 0 || cy_off < 0 ||
             cx_off + cin > cs_x || cy_off + cout > cs_y || act < 0 || act > 3);
}
}  // namespace

extern "C" size_t vstab_conv_dgrad_workspace_bytes(int B, int Ho, int Wo, int cs_g, int cout, int k, int stride, int pad, int Hi, int Wi,
                                                   int cs_x, int cx_off, int cin, int accumulate)
{
    GemmConvPlan d;
    if (!dgrad_plan(B, Ho, Wo, cs_g, cout, k, stride, pad, Hi, Wi, cs_x, cx_off, cin, accumulate ? 1 : 0, d)) return 0;
    return gemm_conv_ws(d).total;
}

extern "C" int vstab_conv_dgrad(const float *gout, int B, int Ho, int Wo, int cs_g, int cg_off, int cout, const float *W, const float *bias_in,
                                int k, int stride, int pad, float *dx, int Hi, int Wi, int cs_x, int cx_off, int cin, int accumulate,
                                void *workspace, size_t workspace_bytes, void *stream)
{
    if (!gout || !W || !dx || !workspace) return fail(nullptr, VSTAB_E_STATE, "conv_dgrad: NULL buffer");
    if (const int c = dgrad_geometry_check(B, Ho, Wo, cs_g, cg_off, cout, k, stride, pad, Hi, Wi, cs_x, cx_off, cin)) return c;
    if ((reinterpret_cast<uintptr_t>(gout) & 15) || (reinterpret_cast<uintptr_t>(dx) & 15) || (reinterpret_cast<uintptr_t>(workspace) & 255))
        return fail(nullptr, VSTAB_E_ALIGN, "conv_dgrad: gout / dx must be 16-byte, workspace 256-byte aligned");
    GemmConvPlan d;
    if (!dgrad_plan(B, Ho, Wo, cs_g, cout, k, stride, pad, Hi, Wi, cs_x, cx_off, cin, accumulate ? 1 : 0, d))
        return fail(nullptr, VSTAB_E_SHAPE, "conv_dgrad: unsupported geometry");
    return run_gemm_conv("conv_dgrad", d, gout + cg_off, (unsigned)((long long)B * Ho * Wo * cs_g * 4 - (long long)cg_off * 4), W, bias_in, dx,
                         workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" size_t vstab_conv_forward_workspace_bytes(int B, int Hi, int Wi, int cs_x, int cin, int k, int stride, int pad, int cout, int cs_y,
                                                     int cy_off, int act, int Ho, int Wo)
{
    GemmConvPlan d;
    if (!fwd_plan(B, Hi, Wi, cs_x, cin, k, stride, pad, cout, cs_y, cy_off, act, Ho, Wo, d)) return 0;
    return gemm_conv_ws(d).total;
}

extern "C" int vstab_conv_forward(const float *x, int B, int Hi, int Wi, int cs_x, int cx_off, int cin, const float *W, const float *bias_in,
                                  int k, int stride, int pad, float *y, int Ho, int Wo, int cs_y, int cy_off, int cout, int act,
                                  void *workspace, size_t workspace_bytes, void *stream)
{
    if (!x || !W || !y || !workspace) return fail(nullptr, VSTAB_E_STATE, "conv_forward: NULL buffer");
    if (!forward_shape_ok(B, Hi, Wi, cs_x, cx_off, cin, k, stride, pad, cs_y, cy_off, cout, act))
        return fail(nullptr, VSTAB_E_SHAPE, "conv_forward: bad shape");
    if ((cx_off & 3) || (cy_off & 3) || (reinterpret_cast<uintptr_t>(x) & 15) || (reinterpret_cast<uintptr_t>(workspace) & 255))
        return fail(nullptr, VSTAB_E_ALIGN, "conv_forward: channel offsets multiples of 4, x 16-byte, workspace 256-byte aligned");
    GemmConvPlan d;
    if (!fwd_plan(B, Hi, Wi, cs_x, cin, k, stride, pad, cout, cs_y, cy_off, act, Ho, Wo, d))
        return fail(nullptr, VSTAB_E_SHAPE, "conv_forward: unsupported geometry");
    return run_gemm_conv("conv_forward", d, x + cx_off, (unsigned)((long long)B * Hi * Wi * cs_x * 4 - (long long)cx_off * 4), W, bias_in, y,
                         workspace, workspace_bytes, (hipStream_t)stream);
}

// Host-only view of plan_forward / plan_dgrad (no HIP call; vstab.h gives the layout of `out`).  x is the image-side tensor (the forward's
// input, the input gradient's dx), y the output side (the forward's y, gout); c_off the channel offset of the tensor the launches write.
extern "C" int vstab_host_train_conv_plan(int dgrad, int B, int Hi, int Wi, int cs_x, int cin, int k, int stride, int pad, int Ho, int Wo,
                                          int cs_y, int cout, int c_off, int act, int32_t *out, int cap, int32_t *table, long long table_cap)
{
    if (!out) return fail(nullptr, VSTAB_E_STATE, "train_conv_plan: NULL buffer");
    GemmConvPlan d{};
    std::vector<int32_t> tbl;
    if (dgrad) {
        if (const int c = dgrad_geometry_check(B, Ho, Wo, cs_y, 0, cout, k, stride, pad, Hi, Wi, cs_x, c_off, cin)) return c;
        if (!plan_dgrad(B, Ho, Wo, cs_y, cout, k, stride, pad, Hi, Wi, cs_x, c_off, cin, act ? 1 : 0, d, tbl))
            return fail(nullptr, VSTAB_E_SHAPE, "conv_dgrad: unsupported geometry");
    } else {
        if (!forward_shape_ok(B, Hi, Wi, cs_x, 0, cin, k, stride, pad, cs_y, c_off, cout, act))
            return fail(nullptr, VSTAB_E_SHAPE, "conv_forward: bad shape");
        if (c_off & 3) return fail(nullptr, VSTAB_E_ALIGN, "conv_forward: channel offsets multiples of 4");
        if (!plan_forward(B, Hi, Wi, cs_x, cin, k, stride, pad, cout, cs_y, c_off, act, Ho, Wo, d, tbl))
            return fail(nullptr, VSTAB_E_SHAPE, "conv_forward: unsupported geometry");
    }
    const int nl = d.nsub ? d.nsub : 1;
    int need = 7;
    for (int s = 0; s < nl; ++s) need += 8 + 12 * (d.nsub ? d.sp[s] : d.p).nphase;
    if (cap < need) return fail(nullptr, VSTAB_E_NOMEM, "train_conv_plan: need %d ints", need);
    if (table && table_cap < (long long)tbl.size()) return fail(nullptr, VSTAB_E_NOMEM, "train_conv_plan: need %zu table entries", tbl.size());
    const size_t ws256 = gemm_conv_ws(d).total / 256;
    if (std::max({d.packed_floats, d.part_floats, ws256}) > 0x7fffffffu) return fail(nullptr, VSTAB_E_SHAPE, "train_conv_plan: sizes beyond int32");
    const int head[7] = {nl, (int)d.packed_floats, (int)d.part_floats, d.blocked_K, d.tbl_nfast ? 1 : 0, (int)ws256, (int)tbl.size()};
    int32_t *o = std::copy(head, head + 7, out);
    for (int s = 0; s < nl; ++s) {
        const ConvParams &p = d.nsub ? d.sp[s] : d.p;
        const int v[8] = {p.nphase, (int)(d.nsub ? d.stile[s] : d.tile), d.vec4 ? 1 : 0, p.ksplit, p.Mmax, p.N, p.Npad, (int)(d.nsub ? d.soff[s] : 0)};
        o = std::copy(v, v + 8, o);
        for (int f = 0; f < p.nphase; ++f) {
            const ConvPhase &ph = p.ph[f];
            const bool own = ph.KH != 0;              // a merged launch's phases carry their own K layout
            const int q[12] = {ph.Hg, ph.Wg, ph.M, ph.off_y, ph.off_x, ph.o_y, ph.o_x, own ? ph.KH : p.KH, own ? ph.NSEG : p.NSEG,
                               own ? ph.SEG : p.SEG, own ? ph.SEGP : p.SEGP, own ? ph.SEG_STRIDE : p.SEG_STRIDE};
            o = std::copy(q, q + 12, o);
        }
    }
    if (table) std::copy(tbl.begin(), tbl.end(), table);
    return need;
}

// ------------------------------------------------------------------------- the first layer on the inference path's row-window kernel
// model.py:807-808 (PadLayer(3) -> Conv2d 7x7 stride 2 VALID, 27 -> 64) with DEVICE-resident raw weights: conv_rowwin_kernel (stream form,
// assembly K loop: 0.92 of the MFMA peak at B=8 512x512, where the generic implicit GEMM reaches 0.73) fed by an operand gathered on
// the device every call -- the host packer's layout, recorded once per geometry as an index table by packing a tensor of indices.
namespace {
struct RowWinPlan { RowWinDesc g; int32_t *tbl; size_t packed_floats; };

// No HIP call.
bool plan_rowwin(int B, int H, int W, int Cin, int cs_w, int cout, int k, int stride, int pad, int cs_y, int cy_off, int act, RowWinPlan &d,
                 std::vector<int32_t> &tbl)
{
    if (cout < 1 || cout > 64 || cs_w < Cin || k < 1 || k > 7 || stride < 1 || pad < 0 || (cy_off & 3) || (cs_y & 3)) return false;
    const int Ho = (H + 2 * pad - k) / stride + 1, Wo = (W + 2 * pad - k) / stride + 1;
    if (Ho < 1 || Wo < 1 || !below_2gib(B, H, W, Cin) || !below_2gib(B, Ho, Wo, cs_y)) return false;
    d.g = rowwin_desc(B, H, W, Cin, k, stride, pad, Ho, Wo, cout, 64, cs_y, cy_off, act);
    if (!d.g.ok) return false;
    const RowWinParams &r = d.g.main;
    // the packer's layout as a gather table: pack a filter whose value at (ky, kx, ci, n) is 1 + its index in the [k,k,cs_w,cout] tensor
    const int lead = rowwin_lead(-pad, Cin);
    d.packed_floats = (size_t)k * (r.SEGP / 32) * 64 * 32;
    std::vector<float> idx((size_t)k * k * Cin * cout), packed(d.packed_floats);
    for (int ky = 0; ky < k; ++ky)
        for (int kx = 0; kx < k; ++kx)
            for (int ci = 0; ci < Cin; ++ci)
                for (int n = 0; n < cout; ++n)
                    idx[(((size_t)ky * k + kx) * Cin + ci) * cout + n] = (float)(1 + (((size_t)ky * k + kx) * cs_w + ci) * cout + n);
    if ((size_t)k * k * cs_w * cout >= (1u << 24)) return false;      // indices must be exact in fp32
    std::vector<double> ones(64, 1.0);
    pack_conv_rowwin(idx.data(), ones.data(), k, k, Cin, cout, 64, lead, r.SEGP, packed.data());
    tbl.assign(packed.begin(), packed.end());
    return true;
}

bool rowwin_plan(int B, int H, int W, int Cin, int cs_w, int cout, int k, int stride, int pad, int cs_y, int cy_off, int act, RowWinPlan &out)
{
    static PlanCache<RowWinPlan, 12> cache(true);
    return cache.get({B, H, W, Cin, cs_w, cout, k, stride, pad, cs_y, cy_off, act}, out, [&](RowWinPlan &d) {
        std::vector<int32_t> tbl;
        return plan_rowwin(B, H, W, Cin, cs_w, cout, k, stride, pad, cs_y, cy_off, act, d, tbl) && (d.tbl = upload_table(tbl));
    });
}

// workspace: the packed operand at 0, then a 64-float bias vector
struct RowWinWs { size_t bias, total; };
RowWinWs rowwin_ws(const RowWinPlan &d)
{
    RowWinWs w{};
    w.bias = a256(d.packed_floats * sizeof(float));
    w.total = w.bias + 512;
    return w;
}
}  // namespace

extern "C" size_t vstab_conv_rowwin_forward_workspace_bytes(int B, int H, int W, int Cin, int cs_w, int cout, int k, int stride, int pad, int cs_y,
                                                            int cy_off, int act)
{
    RowWinPlan d;
    if (!rowwin_plan(B, H, W, Cin, cs_w, cout, k, stride, pad, cs_y, cy_off, act, d)) return 0;
    return rowwin_ws(d).total;
}

extern "C" int vstab_conv_rowwin_forward(const float *x, int B, int H, int W, int Cin, const float *Wf, int cs_w, int cout, const float *bias, int k,
                                         int stride, int pad, float *y, int cs_y, int cy_off, int act, void *workspace, size_t workspace_bytes,
                                         void *stream)
{
    if (!x || !Wf || !y || !workspace) return fail(nullptr, VSTAB_E_STATE, "conv_rowwin_forward: NULL buffer");
    if (act < 0 || act > 2) return fail(nullptr, VSTAB_E_SHAPE, "conv_rowwin_forward: act must be 0, 1 or 2");
    if ((reinterpret_cast<uintptr_t>(x) & 15) || (reinterpret_cast<uintptr_t>(y) & 15) || (reinterpret_cast<uintptr_t>(workspace) & 255))
        return fail(nullptr, VSTAB_E_ALIGN, "conv_rowwin_forward: x and y 16-byte, workspace 256-byte aligned");
    RowWinPlan d;
    if (!rowwin_plan(B, H, W, Cin, cs_w, cout, k, stride, pad, cs_y, cy_off, act, d))
        return fail(nullptr, VSTAB_E_SHAPE, "conv_rowwin_forward: the row-window kernel does not take this geometry");
    const RowWinWs w = rowwin_ws(d);
    if (workspace_bytes < w.total) return fail(nullptr, VSTAB_E_NOMEM, "conv_rowwin_forward: workspace %zu < %zu bytes", workspace_bytes, w.total);
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(nullptr, rowwin_set_attributes());
    float *wpk = reinterpret_cast<float *>(workspace);
    float *b64 = reinterpret_cast<float *>(reinterpret_cast<char *>(workspace) + w.bias);
    HIP_TRY(nullptr, launch_pack_apply(Wf, d.tbl, (long long)d.packed_floats, wpk, st));
    HIP_TRY(nullptr, hipMemsetAsync(b64, 0, 64 * sizeof(float), st));
    if (bias) HIP_TRY(nullptr, hipMemcpyAsync(b64, bias, (size_t)cout * sizeof(float), hipMemcpyDeviceToDevice, st));
    RowWinParams &r = d.g.main, &t = d.g.tail;
    r.in = t.in = x; r.out = t.out = y; r.wpk = t.wpk = wpk; r.bias = t.bias = b64;
    HIP_TRY(nullptr, launch_conv_rowwin(r, st));
    if (d.g.two) HIP_TRY(nullptr, launch_conv_rowwin(t, st));
    return VSTAB_OK;
}

// ------------------------------------------------------------------------- 3x3 stride-1 conv / its input gradient in Winograd form
namespace {
struct WinoPlan {
    ConvParams p;               // the 16-phase 1x1 GEMM over the transformed tiles
    size_t phase_floats;        // packed floats per position
    int K, N, TH, TW;
};

// (host data only: the plan is the same on every device)
bool wino_plan(int B, int H, int W, int K, int N, WinoPlan &out)
{
    static PlanCache<WinoPlan, 5> cache(false);
    return cache.get({B, H, W, K, N}, out, [&](WinoPlan &d) {
        if ((K & 31) || (N & 63)) return false;
        d.K = K; d.N = N; d.TH = (H + 1) / 2; d.TW = (W + 1) / 2;
        if ((long long)B * 16 * d.TH * d.TW * std::max(K, N) * 4 >= 0x80000000LL) return false;
        d.p = conv_desc_wino_gemm(B, H, W, K, N);
        d.phase_floats = (size_t)klayout_run(1, 1, K).ktiles() * N * 32;
        return true;
    });
}

// workspace: the Winograd-domain filter Wt [16][K][N] at 0, its packed form, the transformed tiles V [B][16 TH][TW][K], the products
// M [..][N], a zero bias for the GEMM
struct WinoWs { size_t wpk, V, M, bz, total; };
WinoWs wino_ws(const WinoPlan &d, int B)
{
    const size_t tiles = (size_t)B * 16 * d.TH * d.TW;
    WinoWs w{};
    w.wpk = a256((size_t)16 * d.K * d.N * 4);
    w.V = w.wpk + a256(16 * d.phase_floats * 4);
    w.M = w.V + a256(tiles * d.K * 4);
    w.bz = w.M + a256(tiles * d.N * 4);
    w.total = w.bz + a256((size_t)d.N * 4) + 256;
    return w;
}
}  // namespace

extern "C" size_t vstab_conv3x3_winograd_workspace_bytes(int B, int H, int W, int cin, int cout, int transpose)
{
    WinoPlan d;
    const int K = transpose ? cout : cin, N = transpose ? cin : cout;
    if (B < 1 || H < 1 || W < 1 || !wino_plan(B, H, W, K, N, d)) return 0;
    return wino_ws(d, B).total;
}

extern "C" int vstab_conv3x3_winograd(const float *x, int B, int H, int W, int cs_x, int cx_off, const float *Wf, int cin, int cout, int transpose,
                                      const float *bias, float *y, int cs_y, int cy_off, int act, void *workspace, size_t workspace_bytes,
                                      void *stream)
{
    if (!x || !Wf || !y || !workspace) return fail(nullptr, VSTAB_E_STATE, "conv3x3_winograd: NULL buffer");
    const int K = transpose ? cout : cin, N = transpose ? cin : cout;             // reduction / output channels of this call
    if (B < 1 || H < 1 || W < 1 || cin < 1 || cout < 1 || cx_off < 0 || cy_off < 0 || cx_off + K > cs_x || cy_off + N > cs_y ||
        (act != 0 && act != 1 && act != 3))
        return fail(nullptr, VSTAB_E_SHAPE, "conv3x3_winograd: bad shape");
    if ((cs_x & 3) || (cx_off & 3) || (cs_y & 3) || (cy_off & 3) || (reinterpret_cast<uintptr_t>(x) & 15) || (reinterpret_cast<uintptr_t>(y) & 15) ||
        (reinterpret_cast<uintptr_t>(workspace) & 255))
        return fail(nullptr, VSTAB_E_ALIGN, "conv3x3_winograd: strides / offsets multiples of 4, 16-byte tensors, 256-byte workspace");
    WinoPlan d;
    if (!wino_plan(B, H, W, K, N, d)) return fail(nullptr, VSTAB_E_SHAPE, "conv3x3_winograd: needs K %% 32 == 0, N %% 64 == 0 and < 2 GiB per tensor");
    const WinoWs w = wino_ws(d, B);
    if (workspace_bytes < w.total) return fail(nullptr, VSTAB_E_NOMEM, "conv3x3_winograd: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(nullptr, conv_set_attributes());
    char *ws = reinterpret_cast<char *>(workspace);
    float *Wt = reinterpret_cast<float *>(ws), *wpk = reinterpret_cast<float *>(ws + w.wpk);
    float *V = reinterpret_cast<float *>(ws + w.V), *M = reinterpret_cast<float *>(ws + w.M), *bz = reinterpret_cast<float *>(ws + w.bz);
    HIP_TRY(nullptr, launch_wino_weights(Wf, cin, cout, transpose, Wt, st));
    HIP_TRY(nullptr, launch_pack_blocked(Wt, K, N, N, 16, wpk, st));           // 16 x [K][N] -> 16 x [K/32][N][32]
    HIP_TRY(nullptr, hipMemsetAsync(bz, 0, (size_t)N * sizeof(float), st));
    HIP_TRY(nullptr, launch_wino_input(x, B, H, W, cs_x, cx_off, K, V, st));
    ConvParams p = d.p;
    p.in = V; p.out = M; p.wpk = wpk; p.bias = bz; p.partial = nullptr;
    HIP_TRY(nullptr, launch_conv(p, TILE_128x64, true, st));
    HIP_TRY(nullptr, launch_wino_output(M, B, H, W, N, bias ? bias : bz, act, y, cs_y, cy_off, st));
    return VSTAB_OK;
}

// ------------------------------------------------------------------------- filter gradient of a 3x3 stride-1 conv in Winograd form
extern "C" size_t vstab_conv3x3_winograd_wgrad_workspace_bytes(int B, int H, int W, int cin, int cout)
{
    WgradParams p; int TH, TW;
    if (!wino_wgrad_shape(B, H, W, cin, cout, p, TH, TW)) return 0;
    return wino_wgrad_ws((size_t)B * TH * TW, cin, cout, p.ksplit).total;
}

extern "C" int vstab_conv3x3_winograd_wgrad(const float *x, int B, int H, int W, int cs_x, int cx_off, int cin, const float *gout, int cs_g,
                                            int cg_off, int cout, float *dW, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!x || !gout || !dW || !workspace) return fail(nullptr, VSTAB_E_STATE, "conv3x3_winograd_wgrad: NULL buffer");
    if (cx_off < 0 || cg_off < 0 || cx_off + cin > cs_x || cg_off + cout > cs_g)
        return fail(nullptr, VSTAB_E_SHAPE, "conv3x3_winograd_wgrad: bad channel slices");
    WgradParams p; int TH, TW;
    if (!wino_wgrad_shape(B, H, W, cin, cout, p, TH, TW))
        return fail(nullptr, VSTAB_E_SHAPE, "conv3x3_winograd_wgrad: needs channel counts that are multiples of 4 and < 2 GiB per tensor");
    if ((cs_x & 3) || (cx_off & 3) || (cs_g & 3) || (cg_off & 3) || (reinterpret_cast<uintptr_t>(x) & 15) || (reinterpret_cast<uintptr_t>(gout) & 15) ||
        (reinterpret_cast<uintptr_t>(workspace) & 255))
        return fail(nullptr, VSTAB_E_ALIGN, "conv3x3_winograd_wgrad: strides / offsets multiples of 4, 16-byte tensors, 256-byte workspace");
    const size_t T = (size_t)B * TH * TW;
    const WinoWgradWs w = wino_wgrad_ws(T, cin, cout, p.ksplit);
    if (workspace_bytes < w.total) return fail(nullptr, VSTAB_E_NOMEM, "conv3x3_winograd_wgrad: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    char *ws = reinterpret_cast<char *>(workspace);
    float *V = reinterpret_cast<float *>(ws), *dM = reinterpret_cast<float *>(ws + w.dM), *dU = reinterpret_cast<float *>(ws + w.dU);
    p.partial = reinterpret_cast<float *>(ws + w.partial);
    HIP_TRY(nullptr, launch_wino_input(x, B, H, W, cs_x, cx_off, cin, V, st, true));           // V  [16][T][cin]
    HIP_TRY(nullptr, launch_wino_outgrad(gout, B, H, W, cs_g, cg_off, cout, dM, st));            // dM [16][T][cout]
    // 16 independent reductions dU_xi [cin x cout] = V_xi^T [cin x T] . dM_xi [T x cout]: the weight-gradient kernel's batched form over
    // a 1x1 "image" of T pixels
    p.ptab = wgrad_pixel_table(1, (int)T, 1, cin, (int)T, 1, 1, 0, st);
    if (!p.ptab) return fail(nullptr, VSTAB_E_NOMEM, "conv3x3_winograd_wgrad: cannot build the pixel table");
    p.x = V; p.g = dM; p.dW = dU;
    p.x_bytes = (unsigned)(T * cin * 4); p.g_bytes = (unsigned)(T * cout * 4);
    p.x_bstride = (long long)(T * cin); p.g_bstride = (long long)(T * cout);
    p.accumulate = 0;
    HIP_TRY(nullptr, launch_wgrad(p, st));
    HIP_TRY(nullptr, launch_wino_filter_grad(dU, cin, cout, dW, st));
    return VSTAB_OK;
}
