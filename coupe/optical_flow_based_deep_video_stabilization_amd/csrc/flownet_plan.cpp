// The launch plan of the FlowNetS pyramid: the split-K / tile / Winograd cost model, make_plan over the net table (flownet_plan.h),
// chunking, and the views of a plan that need no GPU (vstab_workspace_*, vstab_host_*).
#include <cmath>
#include <cstdlib>
#include <memory>
#include <new>

#include "flownet_plan.h"

using namespace vstab;

bool level_sizes(int H, int W, int *eh, int *ew)
{
    int h = H, w = W;
    for (int i = 0; i < 10; ++i) {
        h = (h + 2 * NET[i].p - NET[i].k) / NET[i].s + 1;
        w = (w + 2 * NET[i].p - NET[i].k) / NET[i].s + 1;
        if (h < 1 || w < 1) return false;
        eh[i] = h; ew[i] = w;
    }
    // deconv output_shape := skip size needs ceil(out/2) == in
    for (int l = 0; l < 4; ++l)
        if ((eh[LVL_ENC[l + 1]] + 1) / 2 != eh[LVL_ENC[l]] || (ew[LVL_ENC[l + 1]] + 1) / 2 != ew[LVL_ENC[l]]) return false;
    return H >= 3 && W >= 3;
}

// Split-K factor from a small cost model instead of a fixed rule.  A launch is `tiles x ks` workgroups on 512 slots
// (256 CUs x 2 co-resident workgroups); a K-tile costs TAU2 when two workgroups share a CU and TAU1 when one has
// the CU to itself, every workgroup pays a fixed prologue/epilogue T0, and splitting adds the combine pass and the
// slab traffic.  Constants calibrated on the cfg1 / B=1 profiles (profiles/README.md, "split-K model").
static double split_cost_us(long long tiles, int KT, int ks, double slab_bytes, int BN, int BM, int *ks_eff_out)
{
    // 64-row tiles cost half a 128-row tile per K-tile when few workgroups run (measured), a little more than half
    // on a full chip (1.5x the LDS fragment reads per MFMA), so large layers keep the 128-row tile
    const double TAU2 = 4.2 * (BN >= 128 ? 1.0 : (BN == 64 ? 0.58 : 0.36)) * (BM == 64 ? 0.55 : 1.0);
    const double TAU1 = 0.525 * TAU2, T0 = 5.0;     // in-situ: 2.10 vs 4.00 us per K-tile (conv4_1), 2.20 vs 4.19 (conv4); with the assembly K loop
                                                    // 1.87 vs 3.52: same ratio, and 3.55 / 0.53 / T0 3..11 pick the same splits at B=8 512x512 (r03k sweep)
    // bytes per us for the slab traffic: slabs that stay in the L2s (32 MB across the 8 XCDs; one sample's) move at ~12 TB/s, a launch's
    // worth beyond that goes through the Infinity Cache / HBM (round 5 A/B, profiles/ab_r05t_slab_bandwidth.txt: B=8 512x512 conv5 /
    // deconv5 / deconv4 with 34 / 34 / 17 MB of slabs at split 8 / 8 / 4 are faster at 4 / 4 / 2)
    const double BW = slab_bytes * ((KT + ((KT + ks - 1) / ks) - 1) / ((KT + ks - 1) / ks)) > 16e6 ? 5.0e6 : 1.2e7;
    const int kts = (KT + ks - 1) / ks, ks_eff = (KT + kts - 1) / kts;
    const long long blocks = tiles * ks_eff, full = blocks / 512, rem = blocks % 512;
    double t = (double)full * (kts * TAU2 + T0);
    if (rem > 256) t += kts * TAU2 + T0;
    else if (rem > 0) t += kts * TAU1 + T0;
    if (ks_eff > 1) t += 6.0 + (2.0 * ks_eff + 1.0) * slab_bytes / BW;
    *ks_eff_out = ks_eff;
    return t;
}

static double best_split(const ConvParams &p, int BN, int BM, int *ks_out)
{
    const int KT = p.KH * p.NSEG * (p.SEGP / 32);
    const long long tiles = (long long)((p.Mmax + BM - 1) / BM) * (p.Npad / BN) * p.nphase;
    int best = 1, dummy;
    double best_t = split_cost_us(tiles, KT, 1, 0.0, BN, BM, &dummy);
    *ks_out = 1;
    if ((p.N & 3) != 0 || tiles >= 2048) return best_t;
    const double slab = (double)p.Mmax * p.nphase * p.Npad * 4.0;
    const int cap = std::min(64, std::max(1, KT / 3));
    for (int ks = 2; ks <= cap; ++ks) {
        int eff;
        const double t = split_cost_us(tiles, KT, ks, slab, BN, BM, &eff);
        if (eff != ks || slab * ks > 768e6) continue;               // only factors that divide the K-tiles evenly enough
        if (t < best_t * 0.995) { best_t = t; best = ks; }          // prefer the smaller factor on ties
    }
    *ks_out = best;
    return best_t;
}

void choose_split(ConvParams &p, int BN, int BM)
{
    int ks;
    best_split(p, BN, BM, &ks);
    p.ksplit = ks;
}

// Tile + split-K for a 128-column layer: small-M layers (one sample, the 1/32 and 1/64 levels) waste most of a
// 128-row tile and become fixed-overhead / weight-streaming bound; the 64x128 variant halves the MFMA work per K-tile
// there (B=1 384x512: conv5..deconv5 29-36 us -> 21-27 us each in tools/conv_bench).
ConvTile choose_tile_split(ConvParams &p, ConvTile tile, bool vec4)
{
    const int BN = tile == TILE_128x128 ? 128 : (tile == TILE_128x64 ? 64 : 32);
    int ks128;
    const double t128 = best_split(p, BN, 128, &ks128);
    p.ksplit = ks128;
    if (tile != TILE_128x128 || !vec4 || !conv_uses_lds_dma(tile, vec4)) return tile;
    int ks64;
    const double t64 = best_split(p, 128, 64, &ks64);
    if (t64 < 0.95 * t128) { p.ksplit = ks64; return TILE_64x128; }
    return tile;
}

// Few rows per phase (one sample's 1/32 and 1/64 levels, the first decoder steps): the layer is a weight stream (conv_skinny.hip).
// Returns true and sets p.ksplit to that kernel's own factor.
bool choose_skinny(ConvParams &p, bool vec4, unsigned flags)
{
    if (flags & VSTAB_PLAN_NO_SKINNY) return false;
    if (!conv_skinny_applicable(p, vec4)) return false;
    p.ksplit = conv_skinny_split(p);
    return true;
}

// does a 3x3 stride-1 pad-1 layer run in Winograd form?  Two extra HBM passes and two more launches: pays once the Winograd-domain
// GEMM issues a GFLOP or two (measured: B=8 512x512 every encoder stage gains, 20..96 us; one 384x512 sample -- 1.61 GFLOP per stage -- lost
// 2..5 % in rounds 2-3 and GAINS 2.5 % of the frame since the stream GEMMs and one-workgroup-per-CU plans of rounds 4-5: conv3_1 / conv4_1
// 38.4 / 37.1 -> 24.2 / 25.2 us and their split-K combines gone (profiles/ab_r05k_winograd_threshold.txt); one 256x256 sample, 0.54 GFLOP per
// stage, still loses 4 %)
bool wino_applies(int B, int H, int W, int cin, int cout)
{
#ifdef VSTAB_HARNESS
    static const bool wino_on = getenv("VSTAB_NO_WINOGRAD") == nullptr;       // A/B switch of the tuning harness builds
    if (!wino_on) return false;
#endif
    if ((cin & 31) || (cout & 127)) return false;                  // whole K tiles, 128x64 output tiles
    const long long TH = (H + 1) / 2, TW = (W + 1) / 2;
    if ((long long)B * 16 * TH * TW * std::max(cin, cout) * 4 >= 0x80000000LL) return false;
#ifndef VSTAB_WINO_MIN_FLOPS
#define VSTAB_WINO_MIN_FLOPS 1.5e9       // (A/B builds: scripts/build_variant_lib.sh -DVSTAB_WINO_MIN_FLOPS=...)
#endif
    return 32.0 * B * TH * TW * cin * cout >= VSTAB_WINO_MIN_FLOPS;
}

// does refinement level l's transposed convolution run in Winograd F(2x2,2x2) form?  9/16 of the multiply-adds, against two more HBM
// passes (V and M), one more launch, a reduction of only Cin (25 / 33 K-tiles per workgroup instead of 100 / 132) and a ragged tile
// grid (one more tile per axis than Hin/2).  Decided with the cost model that picks the split-K factors: the direct launch's modelled
// time `t_direct_us` against the 9-position GEMM's (on 128- or 64-row tiles, whichever the model prefers: *tile_out) plus the two
// transforms at the bandwidth they measure (4.5 TB/s over input + V + M + output; profiles/README.md r06).  Measured: at B=8 512x512
// deconv3 gains a little (-12 us of 200) and deconv4 would lose (336 workgroups on 512 slots: as long as the direct form) -- the model
// says the same; at 16 x 720p / 8 x 1080p per chunk deconv4 and deconv3 take 0.60 / 0.63 of their direct time and the step -3.7 % / -2.2 %.
// deconv2 (Cin 386 -> 64: 13 K-tiles, N = 256, V and M larger than the layer's own tensors) is not built.
bool wdec_applies(int l, int B, const WdecGeom &g, int Hi, int Wi, int Ho, int Wo, int cs_in, int cout, double t_direct_us, int ks_direct, bool force,
                  ConvTile *tile_out)
{
    *tile_out = TILE_128x128;
#ifdef VSTAB_HARNESS
    static const bool wdec_on = getenv("VSTAB_NO_WDEC") == nullptr;           // A/B switch of the tuning harness builds
    if (!wdec_on) return false;
#endif
    if (l < 0 || l > 2 || (cs_in & 3) || ((4 * cout) & 127) || 4 * cout > 2048) return false;     // (2048 = the zero bias the GEMMs share)
    if ((long long)B * 9 * g.NTy * g.NTx * std::max(cs_in, 4 * cout) * 4 >= 0x80000000LL) return false;
    const int KT = round_up(cs_in, 32) / 32;
    double best = 1e30;
    for (int BM : {128, 64}) {
        long long tiles = 0;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) tiles += ((long long)B * g.nty[i] * g.ntx[j] + BM - 1) / BM;
        int eff;
        const double t = split_cost_us(tiles * (4 * cout / 128), KT, 1, 0.0, 128, BM, &eff);
        if (t < best) { best = t; *tile_out = BM == 128 ? TILE_128x128 : TILE_64x128; }
    }
    if (force) return true;                                                   // VSTAB_PLAN_FORCE_WDEC: small test shapes
    const double plane = (double)B * g.NTy * g.NTx;
    const double bytes = 4.0 * ((double)B * Hi * Wi * cs_in + 9.0 * plane * cs_in + 9.0 * plane * 4.0 * cout + (double)B * Ho * Wo * cout);
#ifndef VSTAB_WDEC_MARGIN
#define VSTAB_WDEC_MARGIN 0.92           // (A/B builds: scripts/build_variant_lib.sh -DVSTAB_WDEC_MARGIN=...)
#endif
    // a direct launch the model splits in K is a small one (B=8 512x512: deconv5 / deconv4, split 4 / 2): the model prices those 20-25 %
    // too high (measured 71 / 133 us against 89 / 163) and the ragged 9-position grid quantises badly on 512 slots -- they stay direct
    if (ks_direct > 1) return false;
    return best + bytes / 4.5e6 + 3.0 < VSTAB_WDEC_MARGIN * t_direct_us;
}

bool fill_plain_conv(ConvParams &p, ConvTile &tile, bool &vec4, int B, int Hi, int Wi, int cin, int cs_in, int k, int stride,
                     int pad, int cout, int cs_out, int c_off, int act)
{
    const int Ho = (Hi + 2 * pad - k) / stride + 1, Wo = (Wi + 2 * pad - k) / stride + 1;
    if (Ho < 1 || Wo < 1 || cs_in < cin) return false;
    tile = default_tile(cout);
    p = conv_desc_plain(B, Hi, Wi, cin, cs_in, k, stride, pad, Ho, Wo, cout, padded_cols(cout), cs_out, c_off, act);
    vec4 = (cs_in % 4 == 0) && (p.SEG % 4 == 0);
    if (!vec4 && tile != TILE_128x64) return false;        // the dword-gather variant exists for 128x64 only
    if ((long long)B * Hi * Wi * cs_in * 4 >= 0x80000000LL || (long long)B * Ho * Wo * cs_out * 4 >= 0x80000000LL) return false;
    tile = choose_tile_split(p, tile, vec4);
    return true;
}

static int max_chunk(int B, int H, int W, int Cin);

bool make_plan(int B, int H, int W, int Cin, Plan &pl, const PlanPin *pin)
{
    if (B < 1 || Cin < 1 || Cin > 4096) return false;
    pl.B = B; pl.H = H; pl.W = W; pl.Cin = Cin;
    if (!level_sizes(H, W, pl.eh, pl.ew)) return false;
    const unsigned flags = pin ? pin->flags : 0u;
    // a pinned plan batch: the decisions come from the plan of (one chunk of) that batch
    std::unique_ptr<Plan> ref;
    if (pin && pin->batch > 0) {
        if (B > pin->batch) return false;
        const int cmax = max_chunk(pin->batch, H, W, Cin);
        if (cmax < 1) return false;
        const int nch = (pin->batch + cmax - 1) / cmax, rb = (pin->batch + nch - 1) / nch;
        if (B > rb) return false;                       // callers process a pinned batch in chunks of rb (vstab_flownets_forward)
        if (B != rb) {
            ref.reset(new (std::nothrow) Plan);
            PlanPin unpinned; unpinned.flags = flags;
            if (!ref || !make_plan(rb, H, W, Cin, *ref, &unpinned)) return false;
        }
    }
    // every tensor must stay below 2^31 BYTES: the kernels address through buffer descriptors with
    // 32-bit byte offsets and use 0xC0000000 as the "reads as zero" offset (larger batches are
    // processed in chunks by vstab_flownets_forward)
    const long long lim = (1LL << 29) - 1;
    if ((long long)B * H * W * Cin > lim) return false;

    for (int b = 0; b < N_BUF; ++b) {
        const long long n = (long long)B * pl.buf_h(b) * pl.buf_w(b) * BUFS[b].cs;
        if (n > lim) return false;
        pl.bytes[b] = (size_t)n * 4;
    }
    // ticket words of the in-launch split-K reductions (conv_skinny.hip): per WORKSPACE, so forwards on one context that use distinct
    // workspaces never share them; zeroed at the start of every forward that has such a layer -- by the first layer's own launch
    // (conv_rowwin's first workgroup), or by a memset node when that layer runs on another kernel
    pl.bytes[B_TICKETS] = SKINNY_MAX_TILES * sizeof(unsigned);

    // ---- encoder convs
    size_t partial_floats = 0;
    for (int i = 0; i < 10; ++i) {
        const Layer &e = NET[i];
        ConvParams &p = pl.cp[i];
        const int cin = i == 0 ? Cin : e.cin, cs_in = i == 0 ? Cin : in_buf(e).cs;
        p = conv_desc_plain(B, i == 0 ? H : pl.eh[i - 1], i == 0 ? W : pl.ew[i - 1], cin, cs_in, e.k, e.s, e.p, pl.eh[i], pl.ew[i], e.cout,
                            padded_cols(e.cout), out_buf(e).cs, e.c_off, 1);
        pl.tile[i] = default_tile(e.cout);
        pl.vec4[i] = (p.Cs_in % 4 == 0) && (p.SEG % 4 == 0);
        if (ref) { pl.tile[i] = ref->tile[i]; pl.skinny[i] = ref->skinny[i]; p.ksplit = ref->cp[i].ksplit; }
        else {
            pl.tile[i] = choose_tile_split(p, pl.tile[i], pl.vec4[i]);
            pl.skinny[i] = i > 0 && choose_skinny(p, pl.vec4[i], flags);
            if (pl.skinny[i]) pl.tile[i] = TILE_SKINNY;
        }
        if (p.ksplit > 1) partial_floats = std::max(partial_floats, (size_t)p.ksplit * p.Mmax * p.Npad);
    }
    // ---- the first layer on the bf16 MFMA with three-piece operands (conv1_bf16x3.hip).  It changes the arithmetic of a sample, so it
    // is a pinned decision: taken from the filter's geometry and the plan flags alone, never from the batch or the image size
    pl.conv1_bf16x3 = ref ? ref->conv1_bf16x3
                          : (!(flags & VSTAB_PLAN_CONV1_FP32) && NET[0].cout == 64 && rowwin_segp(-NET[0].p, NET[0].k, Cin) <= 192);
    // ---- Winograd form of the 3x3 stride-1 stages: a 16-phase 1x1 GEMM over the transformed tiles (winograd_ops.hip)
    size_t wino_v = 0, wino_m = 0;
    for (int i = 0; i < 10; ++i) {
        pl.wino[i] = false;
        const Layer &e = NET[i];
        if (e.k != 3 || e.s != 1 || e.p != 1 || pl.skinny[i]) continue;
        if (ref ? !ref->wino[i] : (in_buf(e).cs != e.cin || !wino_applies(B, pl.eh[i], pl.ew[i], e.cin, e.cout))) continue;      // plain input buffer
        const int TH = (pl.eh[i] + 1) / 2, TW = (pl.ew[i] + 1) / 2;
        pl.wcp[i] = conv_desc_wino_gemm(B, pl.eh[i], pl.ew[i], e.cin, e.cout);
        // The reduction is short (K = C_in: 8..32 K-tiles), so a workgroup's prologue and epilogue weigh in.  Stages with at least
        // two full rounds of 128x128 tiles (2 per CU) take those: twice the MFMA work per prologue + epilogue (in situ with the
        // assembly K loop, B=8 512x512: conv3_1 163.5 -> 152 us, conv4_1 138 -> 135.5); smaller stages keep 128x64 tiles, three
        // co-resident workgroups per CU (conv5_1 40 vs 41.3 us, conv6_1 44.5 vs 68.5)
        {
            const long long t128 = 16LL * ((pl.wcp[i].Mmax + 127) / 128) * (e.cout / 128);
            pl.wtile[i] = t128 >= 1024 ? TILE_128x128 : TILE_128x64;         // (a tile shape changes no sum: not pinned)
        }
        wino_v = std::max(wino_v, (size_t)B * 16 * TH * TW * e.cin);
        wino_m = std::max(wino_m, (size_t)B * 16 * TH * TW * e.cout);
        pl.wino[i] = true;
    }
    // ---- decoder transposed convs: 4 phases of a 2x2-tap conv over the whole input pixel, phase (py, px) from input (j + py - 1, i + px - 1)
    for (int l = 0; l < 4; ++l) {
        const Layer &d = dec_layer(l);
        ConvParams &p = pl.cp[10 + l];
        const int off[2] = {-1, 0};
        p = conv_desc_parity4(B, pl.buf_h(d.in), pl.buf_w(d.in), in_buf(d).cs, in_buf(d).cs, 2, off, pl.buf_h(d.out), pl.buf_w(d.out), d.cout,
                              padded_cols(d.cout), out_buf(d).cs, d.c_off, 1);
        pl.tile[10 + l] = default_tile(d.cout);
        pl.vec4[10 + l] = true;
        if (ref) { pl.tile[10 + l] = ref->tile[10 + l]; pl.skinny[10 + l] = ref->skinny[10 + l]; p.ksplit = ref->cp[10 + l].ksplit; }
        else {
            pl.tile[10 + l] = choose_tile_split(p, pl.tile[10 + l], true);
            // (with the two-problem launches a transposed convolution shares its launch with the flow head and its combine with
            // predict_up: the weight-stream kernel's one advantage -- no combine launch -- is gone, so it serves the encoder only)
            pl.skinny[10 + l] = (flags & VSTAB_PLAN_NO_DUAL) ? choose_skinny(p, true, flags) : false;
            if (pl.skinny[10 + l]) pl.tile[10 + l] = TILE_SKINNY;
        }
        if (p.ksplit > 1) partial_floats = std::max(partial_floats, (size_t)p.nphase * p.ksplit * p.Mmax * p.Npad);
        // Winograd F(2x2,2x2) form (an arithmetic-changing decision: pinned like the others); rides in the two-problem launch only
        pl.wdec[l] = false;
        pl.wdg[l] = wdec_geom(p.Hi, p.Wi, p.Ho, p.Wo);
        if (!(flags & (VSTAB_PLAN_NO_DUAL | VSTAB_PLAN_NO_WDEC)) && !pl.skinny[10 + l]) {
            const ConvTile dt = pl.tile[10 + l];
            int ks_d;
            ConvParams pd1 = p;
            const double t_direct = best_split(pd1, dt == TILE_128x64 ? 64 : 128, dt == TILE_64x128 ? 64 : 128, &ks_d);
            ConvTile wt;
            const bool on = wdec_applies(l, B, pl.wdg[l], p.Hi, p.Wi, p.Ho, p.Wo, p.Cs_in, p.N, t_direct, p.ksplit, (flags & VSTAB_PLAN_FORCE_WDEC) != 0, &wt);
            if (ref ? ref->wdec[l] : on) {
                const WdecGeom &g = pl.wdg[l];
                pl.wdcp[l] = conv_desc_wdec_gemm(B, g, p.Cs_in, p.N);
                pl.wdtile[l] = wt;                                               // (a tile shape changes no sum: not pinned)
                wino_v = std::max(wino_v, (size_t)B * 9 * g.NTy * g.NTx * p.Cs_in);
                wino_m = std::max(wino_m, (size_t)B * 9 * g.NTy * g.NTx * 4 * p.N);
                pl.wdec[l] = true;
            }
        }
    }
    pl.bytes[B_WINO_V] = wino_v * 4;
    pl.bytes[B_WINO_M] = wino_m * 4;
    // ---- tap tables: 1x1 conv of the level's (concat) tensor -> 18 (pad 32) columns
    for (int i = 14; i < N_LAYER; ++i) {
        const Layer &t = NET[i];
        ConvParams &p = pl.cp[i];
        const int h = pl.buf_h(t.in), w = pl.buf_w(t.in), cs = in_buf(t).cs;
        p = conv_desc_plain(B, h, w, cs, cs, 1, 1, 0, h, w, 32, 32, out_buf(t).cs, 0, 0);
        pl.tile[i] = TILE_128x32; pl.vec4[i] = true; pl.skinny[i] = false;
        // (predict2's is launched as tap_panel_kernel, tap_panel.hip: its parameters only feed the flop / byte accounting of the reports)
        if (i == 14) continue;
        if (ref) p.ksplit = ref->cp[i].ksplit;
        else choose_split(p, 32);   // A/B on one box: split-K + combine beats 4..256 long-running workgroups by ~90 us/step
        // the tap table runs in the SAME launch as the level's transposed convolution (conv_dual_kernel): their slabs sit side by side
        const ConvParams &d = pl.cp[i - 5];
        const size_t dec_slab = d.ksplit > 1 ? (size_t)d.nphase * d.ksplit * d.Mmax * d.Npad : 0;
        if (p.ksplit > 1) partial_floats = std::max(partial_floats, dec_slab + (size_t)p.ksplit * p.Mmax * p.Npad);
    }
    pl.bytes[B_PARTIAL] = partial_floats * 4;
    size_t off = 0;
    for (int b = 0; b < N_BUF; ++b) {
        pl.off[b] = off;
        off += (pl.bytes[b] + 255) / 256 * 256;
    }
    pl.total = off;
    return true;
}

// Largest batch whose every tensor stays below 2 GiB (0 if even one sample does not fit).
static int max_chunk(int B, int H, int W, int Cin)
{
    Plan pl;
    return largest_fitting(B, [&](int b) { return make_plan(b, H, W, Cin, pl); });
}

int chunk_size(const PlanPin &pin, int B, int H, int W, int Cin)
{
    const int ref = pin.batch > 0 ? pin.batch : B;
    const int cmax = ref >= 1 ? max_chunk(ref, H, W, Cin) : 0;
    if (cmax < 1) return 0;
    const int nch = (ref + cmax - 1) / cmax;
    return std::min(B, (ref + nch - 1) / nch);
}

// ------------------------------------------------------------------------- workspace views
extern "C" int vstab_level_sizes(int H, int W, int32_t *hw20)
{
    int eh[10], ew[10];
    if (!hw20 || !level_sizes(H, W, eh, ew)) return fail(nullptr, VSTAB_E_SHAPE, "unsupported input size %dx%d", H, W);
    for (int i = 0; i < 10; ++i) { hw20[2 * i] = eh[i]; hw20[2 * i + 1] = ew[i]; }
    return VSTAB_OK;
}

extern "C" size_t vstab_workspace_bytes(int B, int H, int W, int Cin)
{
    Plan pl;
    const int chunk = B >= 1 ? max_chunk(B, H, W, Cin) : 0;
    if (chunk < 1 || !make_plan(chunk, H, W, Cin, pl)) { fail(nullptr, VSTAB_E_SHAPE, "unsupported problem %dx%dx%dx%d", B, H, W, Cin); return 0; }
    return pl.total;
}

extern "C" int vstab_set_plan_batch(vstab_ctx *ctx, int batch)
{
    if (!ctx) return fail(nullptr, VSTAB_E_STATE, "set_plan_batch: ctx is NULL");
    if (batch < 0) return fail(ctx, VSTAB_E_SHAPE, "set_plan_batch: batch must be >= 0 (0 = plan for the batch of each call)");
    ctx->plan_batch = batch;
    return VSTAB_OK;
}

extern "C" int vstab_set_plan_flags(vstab_ctx *ctx, unsigned flags)
{
    if (!ctx) return fail(nullptr, VSTAB_E_STATE, "set_plan_flags: ctx is NULL");
    if (flags & ~(unsigned)(VSTAB_PLAN_NO_SKINNY | VSTAB_PLAN_NO_DUAL | VSTAB_PLAN_NO_TAIL | VSTAB_PLAN_NO_WDEC | VSTAB_PLAN_FORCE_WDEC | VSTAB_PLAN_CONV1_FP32 |
                           VSTAB_PLAN_NO_WINO_STREAM)) return fail(ctx, VSTAB_E_SHAPE, "set_plan_flags: unknown flag bits 0x%x", flags);
    ctx->plan_flags = flags;
    return VSTAB_OK;
}

extern "C" size_t vstab_workspace_bytes_ctx(const vstab_ctx *ctx, int B, int H, int W, int Cin)
{
    Plan pl;
    const PlanPin pin = pin_of(ctx);
    if (pin.batch > 0 && B > pin.batch) { fail(nullptr, VSTAB_E_SHAPE, "batch %d exceeds the pinned plan batch %d", B, pin.batch); return 0; }
    const int chunk = B >= 1 ? chunk_size(pin, B, H, W, Cin) : 0;
    if (chunk < 1 || !make_plan(chunk, H, W, Cin, pl, &pin)) { fail(nullptr, VSTAB_E_SHAPE, "unsupported problem %dx%dx%dx%d", B, H, W, Cin); return 0; }
    return pl.total;
}

static int workspace_layout_of(const PlanPin *pin, int chunk, int H, int W, int Cin, vstab_ws_entry *entries, int max_entries)
{
    Plan pl;
    if (!entries || chunk < 1 || !make_plan(chunk, H, W, Cin, pl, pin))
        return fail(nullptr, VSTAB_E_SHAPE, "unsupported problem %dx%dx%dx%d", chunk, H, W, Cin);
    int n = 0;
    for (int b = 0; b < N_BUF && n < max_entries; ++b) {
        vstab_ws_entry &e = entries[n++];
        std::memset(&e, 0, sizeof e);
        std::snprintf(e.name, sizeof e.name, "%s", BUFS[b].name);
        e.offset_bytes = (int64_t)pl.off[b];
        e.n = chunk; e.h = pl.buf_h(b); e.w = pl.buf_w(b); e.c = BUFS[b].c; e.c_stride = BUFS[b].cs;
        if (BUFS[b].level < 0) { e.n = 1; e.h = 1; e.w = (int32_t)std::min<size_t>(pl.bytes[b] / 4, 0x7fffffff); e.c = 1; e.c_stride = 1; }
    }
    return n;
}

extern "C" int vstab_workspace_layout(int B, int H, int W, int Cin, vstab_ws_entry *entries, int max_entries)
{
    return workspace_layout_of(nullptr, B >= 1 ? max_chunk(B, H, W, Cin) : 0, H, W, Cin, entries, max_entries);     // the workspace holds one chunk of the batch
}

extern "C" int vstab_workspace_layout_ctx(const vstab_ctx *ctx, int B, int H, int W, int Cin, vstab_ws_entry *entries, int max_entries)
{
    const PlanPin pin = pin_of(ctx);
    if (pin.batch > 0 && B > pin.batch) return fail(nullptr, VSTAB_E_SHAPE, "batch %d exceeds the pinned plan batch %d", B, pin.batch);
    return workspace_layout_of(&pin, B >= 1 ? chunk_size(pin, B, H, W, Cin) : 0, H, W, Cin, entries, max_entries);
}

// ------------------------------------------------------------------------- host-only views of a plan
// a descriptor as the host-plan views report it: 26 ints, then 7 per phase; returns the count
static int put_desc(const ConvParams &p, int tile, int vec4, const Layer &L, bool alt_form, int32_t *out)
{
    const int v[26] = {p.B, p.Hi, p.Wi, p.Cs_in, p.KH, p.NSEG, p.SEG, p.SEGP, p.SEG_STRIDE, p.s_in, p.s_out, p.Ho, p.Wo,
                       p.Cs_out, p.c_off, p.N, p.Npad, p.act, p.nphase, p.ksplit, p.Mmax, tile, vec4, L.in, L.out, alt_form ? 1 : 0};
    for (int i = 0; i < 26; ++i) out[i] = v[i];
    for (int k = 0; k < p.nphase; ++k) {
        const ConvPhase &ph = p.ph[k];
        const int q[7] = {ph.Hg, ph.Wg, ph.M, ph.off_y, ph.off_x, ph.o_y, ph.o_x};
        for (int i = 0; i < 7; ++i) out[26 + 7 * k + i] = q[i];
    }
    return 26 + 7 * p.nphase;
}

extern "C" int vstab_host_layer_plan(int B, int H, int W, int Cin, int layer, int32_t *out, int cap)
{
    return vstab_host_layer_plan_pinned(0, 0u, B, H, W, Cin, layer, out, cap);
}

extern "C" int vstab_host_layer_plan_pinned(int plan_batch, unsigned flags, int B, int H, int W, int Cin, int layer, int32_t *out, int cap)
{
    Plan pl;
    PlanPin pin; pin.batch = plan_batch; pin.flags = flags;
    if (!out || layer < 0 || layer > 18 || plan_batch < 0 || !make_plan(B, H, W, Cin, pl, &pin))
        return fail(nullptr, VSTAB_E_SHAPE, "layer_plan: bad arguments");
    const ConvParams &p = pl.cp[layer];
    const int need = 26 + 7 * p.nphase;
    if (cap < need) return fail(nullptr, VSTAB_E_NOMEM, "layer_plan: need %d ints", need);
    return put_desc(p, (int)pl.tile[layer], (int)pl.vec4[layer], NET[layer],
                    (layer < 10 && pl.wino[layer]) || (layer >= 10 && layer < 14 && pl.wdec[layer - 10]), out);
}

// the 9-position GEMM of refinement level l's transposed convolution in Winograd F(2x2,2x2) form, whether or not the plan would choose
// it: the fields of vstab_host_layer_plan (26 + 7 per position) followed by the tile geometry {NTy, NTx, nty[3], ntx[3]}
extern "C" int vstab_host_wdec_plan(int B, int H, int W, int Cin, int l, int32_t *out, int cap)
{
    Plan pl;
    if (!out || l < 0 || l > 3 || !make_plan(B, H, W, Cin, pl)) return fail(nullptr, VSTAB_E_SHAPE, "wdec_plan: bad arguments");
    const ConvParams &d = pl.cp[10 + l];
    const WdecGeom g = wdec_geom(d.Hi, d.Wi, d.Ho, d.Wo);
    const ConvParams p = conv_desc_wdec_gemm(B, g, d.Cs_in, d.N);
    const int need = 26 + 7 * 9 + 8;
    if (cap < need) return fail(nullptr, VSTAB_E_NOMEM, "wdec_plan: need %d ints", need);
    put_desc(p, (int)TILE_128x128, 1, dec_layer(l), pl.wdec[l], out);
    const int gg[8] = {g.NTy, g.NTx, g.nty[0], g.nty[1], g.nty[2], g.ntx[0], g.ntx[1], g.ntx[2]};
    for (int i = 0; i < 8; ++i) out[26 + 63 + i] = gg[i];
    return need;
}

extern "C" long long vstab_host_pack_wdec(int l, const float *W, const double *scale, float *wpk, long long cap)
{
    if (!W || !wpk || l < 0 || l > 3) return fail(nullptr, VSTAB_E_SHAPE, "pack_wdec: bad arguments");
    const Layer &d = dec_layer(l);
    return vstab_host_pack_wdec_shape(W, scale, d.cin, in_buf(d).cs, d.cout, wpk, cap);
}

extern "C" long long vstab_host_pack_layer(int Cin, int layer, const float *W, const double *scale, float *wpk,
                                           long long cap)
{
    if (!W || !wpk || layer < 0 || layer > 18 || Cin < 1) return fail(nullptr, VSTAB_E_SHAPE, "pack_layer: bad arguments");
    std::vector<double> ones;
    const Layer &L = NET[layer];
    const int cs_in = layer == 0 ? Cin : in_buf(L).cs, npad = padded_cols(L.cout);
    if (L.kind == L_CONV) {
        const int ci = layer == 0 ? Cin : L.cin;
        const KLayout K = conv_layout(L.k, L.k, ci, cs_in);
        const long long n = (long long)K.ktiles() * npad * 32;
        if (cap < n) return fail(nullptr, VSTAB_E_NOMEM, "pack_layer: need %lld floats", n);
        if (!scale) { ones.assign(npad, 1.0); scale = ones.data(); }
        pack_conv(W, scale, L.k, L.k, ci, cs_in, L.cout, npad, K, wpk);
        return n;
    }
    if (L.kind == L_DECONV) {
        const long long n = 4LL * klayout_deconv(cs_in).ktiles() * npad * 32;
        if (cap < n) return fail(nullptr, VSTAB_E_NOMEM, "pack_layer: need %lld floats", n);
        if (!scale) { ones.assign(npad, 1.0); scale = ones.data(); }
        pack_deconv(W, scale, L.cin, cs_in, L.cout, npad, wpk);
        return n;
    }
    const long long n = (long long)klayout_run(1, 1, cs_in).ktiles() * 32 * 32;
    if (cap < n) return fail(nullptr, VSTAB_E_NOMEM, "pack_layer: need %lld floats", n);
    pack_predict2_table(W, L.cin, cs_in, 32, wpk);
    return n;
}
