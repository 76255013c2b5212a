// Launch descriptors, each built in ONE place.  Host only.  The caller adds the pointers and keeps its own refusals.
//   * ConvParams (vstab_internal.h) of the three problem shapes the implicit-GEMM kernels run: every builder returns a
//     zero-initialised descriptor with the K layout, phases, Mmax, w_off and the buffer-descriptor ranges set and ksplit = 1; the
//     caller decides the split.
//   * RowWinParams of the first layer's row-window kernels (rowwin_desc, at the end).
#pragma once
#include "vstab_internal.h"

// N -> tile -> Npad: 128-column tiles from 128 columns up, 64 above 32, else 32; the packers and the plans must agree on it
inline vstab::ConvTile default_tile(int cout)
{
    return cout >= 128 ? vstab::TILE_128x128 : (cout > 32 ? vstab::TILE_128x64 : vstab::TILE_128x32);
}
inline int tile_cols(vstab::ConvTile t)
{
    return (t == vstab::TILE_128x128 || t == vstab::TILE_64x128) ? 128 : ((t == vstab::TILE_128x64 || t == vstab::TILE_64x64) ? 64 : 32);
}
inline int padded_cols(int cout, vstab::ConvTile t) { return vstab::round_up(cout, tile_cols(t)); }
inline int padded_cols(int cout) { return padded_cols(cout, default_tile(cout)); }

// K layout of a kh x kw window over the first cin channels of cs_in-wide pixels: one run per row tap when the pixel is all used
inline vstab::KLayout conv_layout(int kh, int kw, int cin, int cs_in)
{
    return cs_in == cin ? vstab::klayout_run(kh, kw, cs_in) : vstab::klayout_tap(kh, kw, cin, cs_in);
}

// One-phase kh x kw conv: output pixel (j, i) of the Hg x Wg grid reads rows j*s_in + off_y + t and lands at
// (j*s_out + o_y, i*s_out + o_x), channels [c_off, c_off + cout) of a cs_out-wide pixel of the Ho x Wo output.
struct ConvGrid { int Hg, Wg, off_y, off_x, s_out, o_y, o_x; };
vstab::ConvParams conv_desc_phase(int B, int Hi, int Wi, int cin, int cs_in, int kh, int kw, int s_in, const ConvGrid &g, int Ho, int Wo,
                                  int cout, int npad, int cs_out, int c_off, int act);
// ... the plain case: k x k, stride, zero pad, one output pixel per grid point
inline vstab::ConvParams conv_desc_plain(int B, int Hi, int Wi, int cin, int cs_in, int k, int stride, int pad, int Ho, int Wo, int cout,
                                         int npad, int cs_out, int c_off, int act)
{
    return conv_desc_phase(B, Hi, Wi, cin, cs_in, k, k, stride, ConvGrid{Ho, Wo, -pad, -pad, 1, 0, 0}, Ho, Wo, cout, npad, cs_out, c_off, act);
}

// Stride-2 transposed conv as four output-parity phases (phase = 2 py + px) of a taps x taps conv over the input: phase grid
// ceil((Ho - py) / 2) x ceil((Wo - px) / 2), input offset off[parity] on each axis, packed operands one phase after the other.
vstab::ConvParams conv_desc_parity4(int B, int Hi, int Wi, int cin, int cs_in, int taps, const int off[2], int Ho, int Wo, int cout, int npad,
                                    int cs_out, int c_off, int act);

// 1x1 GEMM over P planes stacked along the rows (Winograd domain): plane q has Hg[q] x Wg[q] live tiles at row q * pitch of a
// [B][P * pitch][Wi][cs_in] tensor, its own packed operand, and writes the same place of [B][P * pitch][Wi][cout].
vstab::ConvParams conv_desc_planes(int B, int P, int pitch, int Wi, const int *Hg, const int *Wg, int cs_in, int cout);
// the 16 positions of F(2x2,3x3) over an H x W image, and the 9 of a transposed conv's F(2x2,2x2) (4 cout columns: one per phase)
vstab::ConvParams conv_desc_wino_gemm(int B, int H, int W, int cin, int cout);
vstab::ConvParams conv_desc_wdec_gemm(int B, const vstab::WdecGeom &g, int cs_in, int cout);

// Row-window kernels (conv_rowwin.hip, conv1_bf16x3.hip): k x k, stride, zero pad over all cin channels of the pixel.  main covers the
// whole row, or, when the row is 128 n + (1..64) pixels long and runs on 128-pixel tiles, its n full tiles, and tail (two = true) the
// rest as ONE 64-pixel tile in a launch of its own.  ok = rowwin_geometry_ok(main).  Zero-initialised but for the geometry: the caller
// adds the pointers (and main's clear_words) and keeps its own refusals.
struct RowWinDesc { vstab::RowWinParams main, tail; bool ok, two; };
RowWinDesc rowwin_desc(int B, int H, int W, int cin, int k, int stride, int pad, int Ho, int Wo, int cout, int npad, int cs_out, int c_off,
                       int act);
