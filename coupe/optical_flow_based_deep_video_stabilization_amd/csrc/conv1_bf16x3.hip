// The first layer (model.py:807-809: PadLayer(3) + Conv2d 7x7 s2 VALID + BatchNorm + lrelu on the 27-channel frame stack) on the
// bf16 matrix pipe with fp32 accuracy: the row-window kernel of conv_rowwin.hip (the tile, window and epilogue of rowwin_tile.h) with
// every fp32 operand split into three bf16 pieces.
//
//   x = x1 + x2 + x3 exactly:  x1 = bf16(x), x2 = bf16(x - x1), x3 = bf16(x - x1 - x2)   (round to nearest even; both differences
//   are exact in fp32, and the three 8-bit significands cover fp32's 24)
//   a b  ~  a3 b1 + a2 b2 + a1 b3 + a2 b1 + a1 b2 + a1 b1     (the three products left out are <= 3 * 2^-24 |a b| together)
//
// v_mfma_f32_32x32x16_bf16 issues 16 times the multiply-adds per cycle of v_mfma_f32_32x32x2_f32, bf16 x bf16 products are exact in
// its fp32 accumulators, so the six products cost 6/16 of the fp32 form's matrix time.
//   * weights: split on the host (pack_conv1_bf16x3), three planes per K-group of 16 in the B-fragment layout, read by every wave
//     straight from global memory into registers one K-group ahead (16 B per lane and plane; 504 KB: they live in L2)
//   * inputs: the workgroup's window of one filter row arrives in registers as fp32 (as in conv_rowwin.hip), is split ONCE per
//     element there and stored as three bf16 planes in LDS; lane i's A fragment of K-group g is the 8 consecutive bf16 at
//     pix_step*i + 16 g + 8 h of each plane.  pix_step = 54 elements = 108 bytes: the fragments are 4-byte aligned only, so they are
//     read as four 32-bit words (32 lanes 27 words apart hit 32 distinct banks); a 16-byte DS read off its alignment is replayed.
//   * per K-group the six products go smallest first into the same accumulator, always in the same order: the same bits run to run,
//     whatever the tile height and the batch
//   * one set of planes per workgroup (3 * WLEN * 2 bytes, 42 KB for 128-pixel tiles): the next filter row's fp32 window is in flight
//     in registers under the MFMAs of this one, then barrier, split + store, barrier; two or three workgroups per CU cover the gap
#include "rowwin_tile.h"

namespace vstab {

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

template <int NWIN4, int MB>   // float4 loads per thread per window; 32-pixel blocks per wave (rowwin_tile.h)
__global__ __launch_bounds__(256) void conv1_bf16x3_kernel(const RowWinParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned *planes = reinterpret_cast<unsigned *>(smem);  // [3][WLEN] bf16, addressed in 32-bit words

    const RowWinTile<MB> t = rowwin_tile<MB>(p);
    const int tid = t.tid, wm = t.wm, wn = t.wn, li = t.li, lh = t.lh;
    const int oy = t.row, pix_step = t.pix_step;

    f32x4 wv[NWIN4];
    auto load_window = [&](int ky) { rowwin_load_window(t, p, oy, ky, wv); };
    // the split, once per staged element: three conversions and two (exact) subtractions
    const int plane_w = p.WLEN >> 1;                        // 32-bit words per plane
    auto split_store = [&]() {
#pragma unroll
        for (int j = 0; j < NWIN4; ++j) {
            const int c4 = tid + 256 * j;
            if (4 * c4 < p.WLEN) {
                bf16x4 h, m, l;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float x = wv[j][e];
                    h[e] = (__bf16)x;
                    const float r1 = x - (float)h[e];
                    m[e] = (__bf16)r1;
                    const float r2 = r1 - (float)m[e];
                    l[e] = (__bf16)r2;
                }
                *reinterpret_cast<u32x2 *>(planes + 2 * c4) = __builtin_bit_cast(u32x2, h);
                *reinterpret_cast<u32x2 *>(planes + plane_w + 2 * c4) = __builtin_bit_cast(u32x2, m);
                *reinterpret_cast<u32x2 *>(planes + 2 * plane_w + 2 * c4) = __builtin_bit_cast(u32x2, l);
            }
        }
    };

    // B fragments: packed [K-group][plane][64][2][8] bf16; lane (i,h) of n-block wn owns the 16 bytes (h) of column wn*32+i
    const int KG = p.SEGP >> 4;                             // K-groups per filter row (even: SEGP is a multiple of 32)
    const int NG = p.KH * KG;
    const unsigned *bbase = reinterpret_cast<const unsigned *>(p.wpk) + (wn * 32 + li) * 8 + lh * 4;
    auto load_b = [&](u32x4 (&b)[3], int G) {
        const unsigned *s = bbase + (long long)(G < NG ? G : NG - 1) * (3 * 512);
#pragma unroll
        for (int q = 0; q < 3; ++q) b[q] = *reinterpret_cast<const u32x4 *>(s + q * 512);
    };
    // A fragments: 8 bf16 at pix_step*m + w_a + 16 g + 8 h of every plane, as four words (4-byte aligned: pix_step and w_a are even)
    const int a_w0 = (pix_step * (wm * 32 * MB + li) + p.w_a + 8 * lh) >> 1;
    const int a_w1 = a_w0 + ((pix_step * 32) >> 1);
    auto load_a = [&](u32x4 (&a)[3 * MB], int g) {
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const unsigned *s = planes + q * plane_w + (mb ? a_w1 : a_w0) + 8 * g;
                u32x4 v;
                v.x = s[0]; v.y = s[1]; v.z = s[2]; v.w = s[3];
                a[mb * 3 + q] = v;
            }
    };

    f32x16 acc[MB];
#pragma unroll
    for (int a = 0; a < MB; ++a)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[a][r] = 0.f;

    // one K-group: the six products, smallest first (a = input pieces, b = weight pieces; 1 = high)
    auto mma = [&](const u32x4 (&a)[3 * MB], const u32x4 (&b)[3]) {
        constexpr int PA[6] = {2, 1, 0, 1, 0, 0}, PB[6] = {0, 1, 2, 0, 1, 0};
#pragma unroll
        for (int t = 0; t < 6; ++t)
#pragma unroll
            for (int mb = 0; mb < MB; ++mb)
                acc[mb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a[mb * 3 + PA[t]]),
                                                                  __builtin_bit_cast(bf16x8, b[PB[t]]), acc[mb], 0, 0, 0);
    };

    u32x4 a0[3 * MB], a1[3 * MB], b0[3], b1[3];
    load_window(0);
    load_b(b0, 0);
    split_store();
    __syncthreads();
    int G = 0;
    for (int ky = 0; ky < p.KH; ++ky) {
        const bool more = ky + 1 < p.KH;
        if (more) load_window(ky + 1);
        load_a(a0, 0);
        __builtin_amdgcn_sched_barrier(0);
        // two K-groups per trip with two named fragment sets: the reads of group g+1 are issued before the MFMAs of group g.  (A ring of
        // four weight sets requested three groups ahead measured SLOWER at B=8 512x512: step -1.6 % instead of -5.1 % against the fp32 form:
        // profiles/ab_r07a_conv1_bf16x3.txt)
        for (int g = 0; g < KG; g += 2, G += 2) {
            load_a(a1, g + 1);
            load_b(b1, G + 1);
            __builtin_amdgcn_sched_barrier(0);
            mma(a0, b0);
            __builtin_amdgcn_sched_barrier(0);
            if (g + 2 < KG) load_a(a0, g + 2);
            load_b(b0, G + 2);
            __builtin_amdgcn_sched_barrier(0);
            mma(a1, b1);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (more) {
            __syncthreads();                          // every wave has read its last fragments of this filter row
            split_store();
            __syncthreads();
        }
    }

    rowwin_epilogue(t, p, acc, oy, reinterpret_cast<float *>(smem));       // the planes are free now
}

hipError_t conv1_bf16x3_set_attributes()
{
    return rowwin_set_lds_limits(conv1_bf16x3_kernel<7, 2>, 3 * 7 * 1024 * 2, conv1_bf16x3_kernel<4, 1>, 3 * 4 * 1024 * 2);
}

hipError_t launch_conv1_bf16x3(const RowWinParams &p, hipStream_t stream, hipEvent_t ev_start, hipEvent_t ev_stop)
{
    if (!conv1_bf16x3_geometry_ok(p)) return hipErrorInvalidValue;
    RowWinParams q = p;
    q.asm_loop = 0;
    q.stream_rows = 0;
    return rowwin_launch(q, conv1_bf16x3_kernel<7, 2>, conv1_bf16x3_kernel<4, 1>, (size_t)3 * p.WLEN * 2, stream, ev_start, ev_stop);
}

}  // namespace vstab
