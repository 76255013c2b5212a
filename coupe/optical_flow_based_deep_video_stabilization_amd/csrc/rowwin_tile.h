// What the two row-window kernels (conv_rowwin.hip: fp32 MFMA; conv1_bf16x3.hip: bf16 MFMA on three-piece operands) have in common,
// stated once: the workgroup's tile of one output row, the fp32 window of one filter row, the epilogue, and the host side of a launch.
// Each kernel keeps its own LDS layout of the operands, its fragment loads and its K loop.  For the two .hip files only.
#pragma once
#include <hip/hip_ext.h>

#include "vstab_internal.h"

namespace vstab {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

typedef void (*RowWinKernel)(const RowWinParams);

constexpr unsigned ROWWIN_OOB = 0xC0000000u;      // a byte offset past any buffer range: the load returns zeros

// MB = 32-pixel blocks per wave: 2 -> 128 output pixels per workgroup (wave tile 64 x 32); 1 -> 64 pixels (wave tile 32 x 32) for
// launches that would otherwise put fewer than two workgroups on a CU (one sample at 384x512: 384 workgroups on 256 CUs run as
// two uneven rounds, 91 us; 768 half-size ones are all resident at once)
template <int MB>
struct RowWinTile {
    int tid, wm, wn, li, lh;            // 2x2 waves, wave tile 32*MB (pixels) x 32 (channels); lane = (li, lh)
    int row, ox0, n;                    // first grid coordinate (the output row, or the stream of rows), first output column, sample
    int pix_step, row_floats;           // floats between the windows of neighbouring output pixels; floats of an input row
    int g0;                             // window start, floats from the row start (multiple of 4)
    __amdgpu_buffer_rsrc_t rin;         // the input tensor; an offset out of its range (ROWWIN_OOB) loads zeros
};

template <int MB>
__device__ __forceinline__ RowWinTile<MB> rowwin_tile(const RowWinParams &p)
{
    RowWinTile<MB> t;
    t.tid = threadIdx.x;
    const int lane = t.tid & 63, wave = t.tid >> 6;
    t.wm = wave >> 1; t.wn = wave & 1;
    t.li = lane & 31; t.lh = lane >> 5;
    // XCD-aware order: grid = (row, x tile, sample) so that a remapped XCD range is a band of consecutive output rows, whose
    // 7-row input windows overlap by five rows
    unsigned bx_, by_, bz_;
    xcd_remap(bx_, by_, bz_);
    // a chore for the launches that FOLLOW this one in the forward: the first workgroup zeroes the ticket words of the in-launch split-K
    // reductions (conv_skinny.hip).  As the forward's first launch this kernel finishes before any of them starts (stream order), and the
    // words ride here instead of in a memset node of their own (4.7 us per forward: 1 ... 1.6 % of a one-sample frame)
    if (p.clear_n > 0 && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0)
        for (int i = t.tid; i < p.clear_n; i += 256) p.clear_words[i] = 0u;
    t.row = (int)bx_;
    t.ox0 = p.ox_base + (int)by_ * (64 * MB); t.n = (int)bz_;
    t.pix_step = p.s_in * p.Cs_in;
    t.row_floats = p.Wi * p.Cs_in;
    t.g0 = t.pix_step * t.ox0 + p.e_off - p.w_a;
    t.rin = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.in), 0, p.in_bytes, 0x00020000);
    return t;
}

// 16-byte chunk j of this thread's share of the window (chunk tid + 256 j): g = its first float's offset in the input row; true when
// the chunk lies inside both the row and the window
template <int MB>
__device__ __forceinline__ bool rowwin_chunk(const RowWinTile<MB> &t, const RowWinParams &p, int j, int &g)
{
    const int c4 = t.tid + 256 * j;
    g = t.g0 + 4 * c4;
    return g >= 0 && g < t.row_floats && 4 * c4 < p.WLEN;
}

// the window of filter row ky of output row oy, as fp32 in registers (NWIN4 float4 loads per thread)
template <int NWIN4, int MB>
__device__ __forceinline__ void rowwin_load_window(const RowWinTile<MB> &t, const RowWinParams &p, int oy, int ky, f32x4 (&wv)[NWIN4])
{
    const int iy = oy * p.s_in + p.off_y + ky;
    const bool yok = (unsigned)iy < (unsigned)p.Hi;
    const int rowbase = ((t.n * p.Hi + iy) * p.Wi) * p.Cs_in;      // element offset (< 2^29, checked on the host)
#pragma unroll
    for (int j = 0; j < NWIN4; ++j) {
        int g;
        const bool ok = rowwin_chunk(t, p, j, g) && yok;
        const unsigned off = ok ? (unsigned)(rowbase + g) * 4u : ROWWIN_OOB;
        wv[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(t.rin, off, 0, 0));
    }
}

// accumulator register r of a wave's 32-pixel block mb -> pixel of the tile (the 32x32 MFMA's C layout: col = lane & 31)
template <int MB>
__device__ __forceinline__ int rowwin_acc_pixel(const RowWinTile<MB> &t, int mb, int r)
{
    return t.wm * 32 * MB + mb * 32 + (r & 3) + 8 * (r >> 2) + 4 * t.lh;
}

// Epilogue of the tile of output row oy: + bias, activation, store to channels c_off .. c_off + N.  As in conv_mfma.hip the tile leaves
// through LDS (sC [64 MB][64] floats over the operands, which are free now) as 16-byte stores of whole 256-byte pixel rows instead of
// 32 four-byte store instructions per wave; p.out_vec4 = 0: straight from the registers.
template <int MB>
__device__ __forceinline__ void rowwin_epilogue(const RowWinTile<MB> &t, const RowWinParams &p, const f32x16 (&acc)[MB], int oy, float *sC)
{
    const int col = t.wn * 32 + t.li;
    if (p.out_vec4) {
        constexpr int TP = 64 * MB;                   // pixels of the tile
        __syncthreads();                              // every wave has read its last operands
        const float bv = col < p.N ? p.bias[col] : 0.f;
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
#pragma unroll
            for (int r = 0; r < 16; ++r) sC[rowwin_acc_pixel(t, mb, r) * 64 + col] = acc[mb][r] + bv;
        __syncthreads();
        const float slope = p.act == 1 ? 0.1f : 0.0f;
        float *orow = p.out + ((long long)(t.n * p.Ho + oy) * p.Wo + t.ox0) * p.Cs_out + p.c_off;
#pragma unroll 4
        for (int e = t.tid; e < TP * 16; e += 256) {
            const int px = e >> 4, c4 = (e & 15) * 4;
            if (t.ox0 + px >= p.Wo || c4 >= p.N) continue;
            f32x4 v = *reinterpret_cast<const f32x4 *>(sC + px * 64 + c4);
            if (p.act) {
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = fmaxf(v[i], slope * v[i]);
            }
            float *o = orow + (long long)px * p.Cs_out + c4;
            if (c4 + 4 <= p.N) *reinterpret_cast<f32x4 *>(o) = v;
            else for (int i = 0; c4 + i < p.N; ++i) o[i] = v[i];
        }
    } else if (col < p.N) {
        const float bv = p.bias[col];
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ox = t.ox0 + rowwin_acc_pixel(t, mb, r);
                if (ox < p.Wo) {
                    float v = acc[mb][r] + bv;
                    if (p.act) v = fmaxf(v, (p.act == 1 ? 0.1f : 0.0f) * v);
                    p.out[((long long)(t.n * p.Ho + oy) * p.Wo + ox) * p.Cs_out + p.c_off + col] = v;
                }
            }
    }
}

// ---- host: what the two launchers share.  x tiles of THIS launch, or -1 for a launch window the kernels do not take
inline int rowwin_xtiles(const RowWinParams &p)
{
    const int tile = 64 * p.MB;
    if (p.ox_base < 0 || p.ox_base >= p.Wo || (p.ox_base & 1) || p.ntile_x < 0) return -1;
    return p.ntile_x > 0 ? p.ntile_x : (p.Wo - p.ox_base + tile - 1) / tile;
}

// Launch k72 (128-pixel tiles) or k41 (64-pixel tiles) with lds bytes of dynamic LDS; q carries the launcher's asm_loop and stream_rows.
inline hipError_t rowwin_launch(RowWinParams q, RowWinKernel k72, RowWinKernel k41, size_t lds, hipStream_t stream, hipEvent_t ev_start,
                                hipEvent_t ev_stop)
{
    const int ntx = rowwin_xtiles(q);
    if (ntx < 0 || ((uintptr_t)q.in & 15) != 0) return hipErrorInvalidValue;
    // (row or stream of rows, x tile, sample): see the XCD remap in rowwin_tile
    dim3 grid(q.stream_rows > 0 ? q.Ho / q.stream_rows : q.Ho, ntx, q.B), block(256);
    // the staged epilogue needs 16-byte friendly output rows and the [tile][64] fp32 staging area inside the kernel's LDS
    q.out_vec4 = (((uintptr_t)q.out & 15) == 0 && (q.Cs_out & 3) == 0 && (q.c_off & 3) == 0 && lds >= (size_t)64 * q.MB * 64 * 4) ? 1 : 0;
    const RowWinKernel k = q.MB == 2 ? k72 : k41;
    // timed: timestamps of the kernel's own dispatch packet, no marker packets (see conv_mfma.hip); a launch that is one half of a pair
    // carries only the start or only the stop event
    if (ev_start || ev_stop) hipExtLaunchKernelGGL(k, grid, block, lds, stream, ev_start, ev_stop, 0, q);
    else k<<<grid, block, lds, stream>>>(q);
    return hipGetLastError();
}

// raise the dynamic-LDS limit of the two instantiations, once per process
inline hipError_t rowwin_set_lds_limits(RowWinKernel k72, int bytes72, RowWinKernel k41, int bytes41)
{
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k72), hipFuncAttributeMaxDynamicSharedMemorySize, bytes72);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute(reinterpret_cast<const void *>(k41), hipFuncAttributeMaxDynamicSharedMemorySize, bytes41);
}

}  // namespace vstab
