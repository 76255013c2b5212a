// The launch-descriptor builders (conv_desc.h).
#include <algorithm>
#include <cstring>

#include "conv_desc.h"

using namespace vstab;

namespace {
// everything but the phases: tensors, K layout, columns
ConvParams desc_base(int B, int Hi, int Wi, int cs_in, const KLayout &L, int s_in, int s_out, int Ho, int Wo, int cout, int npad, int cs_out,
                     int c_off, int act, int nphase)
{
    ConvParams p;
    std::memset(&p, 0, sizeof p);
    p.B = B; p.Hi = Hi; p.Wi = Wi; p.Cs_in = cs_in;
    p.KH = L.KH; p.NSEG = L.NSEG; p.SEG = L.SEG; p.SEGP = L.SEGP; p.SEG_STRIDE = L.SEG_STRIDE;
    p.s_in = s_in; p.s_out = s_out; p.Ho = Ho; p.Wo = Wo; p.Cs_out = cs_out; p.c_off = c_off;
    p.N = cout; p.Npad = npad; p.act = act; p.nphase = nphase; p.ksplit = 1;
    // buffer-descriptor ranges (bytes)
    p.in_bytes = (unsigned)std::min<long long>((long long)B * Hi * Wi * cs_in * 4, 0xFFFFFFFFLL);
    p.w_bytes = (unsigned)std::min<long long>((long long)L.ktiles() * npad * 128, 0xFFFFFFFFLL);
    return p;
}

// phase k: an Hg x Wg grid whose packed operand is the k-th of the launch
void set_phase(ConvParams &p, int k, int Hg, int Wg, int off_y, int off_x, int o_y, int o_x)
{
    ConvPhase &ph = p.ph[k];
    ph.Hg = Hg; ph.Wg = Wg; ph.M = p.B * Hg * Wg;
    ph.off_y = off_y; ph.off_x = off_x; ph.o_y = o_y; ph.o_x = o_x;
    ph.w_off = (long long)k * ((long long)p.KH * p.NSEG * (p.SEGP / 32) * p.Npad * 32);
    p.Mmax = std::max(p.Mmax, ph.M);
}
}  // namespace

ConvParams conv_desc_phase(int B, int Hi, int Wi, int cin, int cs_in, int kh, int kw, int s_in, const ConvGrid &g, int Ho, int Wo, int cout,
                           int npad, int cs_out, int c_off, int act)
{
    ConvParams p = desc_base(B, Hi, Wi, cs_in, conv_layout(kh, kw, cin, cs_in), s_in, g.s_out, Ho, Wo, cout, npad, cs_out, c_off, act, 1);
    set_phase(p, 0, g.Hg, g.Wg, g.off_y, g.off_x, g.o_y, g.o_x);
    return p;
}

ConvParams conv_desc_parity4(int B, int Hi, int Wi, int cin, int cs_in, int taps, const int off[2], int Ho, int Wo, int cout, int npad,
                             int cs_out, int c_off, int act)
{
    ConvParams p = desc_base(B, Hi, Wi, cs_in, conv_layout(taps, taps, cin, cs_in), 1, 2, Ho, Wo, cout, npad, cs_out, c_off, act, 4);
    for (int py = 0; py < 2; ++py)
        for (int px = 0; px < 2; ++px) set_phase(p, py * 2 + px, (Ho - py + 1) / 2, (Wo - px + 1) / 2, off[py], off[px], py, px);
    return p;
}

ConvParams conv_desc_planes(int B, int P, int pitch, int Wi, const int *Hg, const int *Wg, int cs_in, int cout)
{
    ConvParams p = desc_base(B, P * pitch, Wi, cs_in, klayout_run(1, 1, cs_in), 1, 1, P * pitch, Wi, cout, cout, cout, 0, 0, P);
    for (int q = 0; q < P; ++q) set_phase(p, q, Hg[q], Wg[q], q * pitch, 0, q * pitch, 0);
    return p;
}

ConvParams conv_desc_wino_gemm(int B, int H, int W, int cin, int cout)
{
    int Hg[16], Wg[16];
    for (int q = 0; q < 16; ++q) { Hg[q] = (H + 1) / 2; Wg[q] = (W + 1) / 2; }
    return conv_desc_planes(B, 16, Hg[0], Wg[0], Hg, Wg, cin, cout);
}

ConvParams conv_desc_wdec_gemm(int B, const WdecGeom &g, int cs_in, int cout)
{
    int Hg[9], Wg[9];
    for (int q = 0; q < 9; ++q) { Hg[q] = g.nty[q / 3]; Wg[q] = g.ntx[q % 3]; }
    return conv_desc_planes(B, 9, g.NTy, g.NTx, Hg, Wg, cs_in, 4 * cout);
}

RowWinDesc rowwin_desc(int B, int H, int W, int cin, int k, int stride, int pad, int Ho, int Wo, int cout, int npad, int cs_out, int c_off,
                       int act)
{
    RowWinDesc d;
    std::memset(&d, 0, sizeof d);
    RowWinParams &r = d.main;
    r.in_bytes = (unsigned)std::min<long long>((long long)B * H * W * cin * 4, 0xFFFFFFFFLL);
    r.B = B; r.Hi = H; r.Wi = W; r.Cs_in = cin; r.KH = k;
    r.SEGP = rowwin_segp(-pad, k, cin);
    r.s_in = stride; r.off_y = -pad;
    r.e_off = -pad * cin - rowwin_lead(-pad, cin);
    r.w_a = ((r.e_off % 4) + 4) % 4;
    r.Ho = Ho; r.Wo = Wo; r.Cs_out = cs_out; r.c_off = c_off; r.N = cout; r.Npad = npad; r.act = act;
    // window of a tile of 64 MB pixels: from the first pixel's run to the end of the last one's
    auto tile = [](RowWinParams &q, int MB) { q.MB = MB; q.WLEN = round_up(q.s_in * q.Cs_in * (64 * MB - 1) + q.w_a + q.SEGP, 4); };
    tile(r, rowwin_mb(B, Ho, Wo));
    d.ok = rowwin_geometry_ok(r);
    const int rem = Wo % 128;
    if (d.ok && r.MB == 2 && Wo > 128 && rem >= 1 && rem <= 64) {
        RowWinParams &t = d.tail;
        t = r;
        tile(t, 1);
        t.ox_base = (Wo / 128) * 128; t.ntile_x = 1;
        d.two = rowwin_geometry_ok(t);
        if (d.two) r.ntile_x = Wo / 128;
    }
    return d;
}
