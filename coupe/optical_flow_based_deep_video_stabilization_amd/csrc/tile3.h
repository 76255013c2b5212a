// The skeleton of the "3-channel tile" kernels (flow_ops.hip: warp, glue, resize, the fused tails; sampler_ops.hip: the
// spatial-transformer family), first measured for tf_warp (profiles/README.md, "r02 warp study"):
//   * a workgroup of 256 threads owns a TH x TW tile of ONE sample's output pixels and every wave instruction works on a
//     WH x WW patch (WH * WW = 64), so the lines a gather touches are a compact 2-D footprint; a thread handles PPT pixels
//     ("passes"), pass j of wave w being patch q = 4 j + w of the tile;
//   * workgroups are numbered through the XCD map: one XCD's L2 sees a contiguous band of tile rows;
//   * results leave through LDS as 16-byte stores of whole tile rows (4-byte stores for 8-bit pixels).
// Stated once here: the shapes, the workgroup's tile (the constructor), a pass's pixel and its prologue (pixel<PARK>: each kernel keeps its
// own parking rule), the staged row store, and the host's tile count / guards.  The tile kernels of sampler_ops.hip and warp_flow_grad.hip
// interleave the prologue with per-pixel work or skip instead of parking, and keep their loops.
#pragma once
#include "vstab_internal.h"

namespace vstab {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
struct __attribute__((packed, aligned(4))) rgb3 { float r, g, b; };

// where a pass beyond the output is parked: the output's origin, the tile's origin, or the nearest output pixel
enum class Park { ORIGIN, TILE, CLAMP };

constexpr int WT_WH = 4, WT_WW = 16, WT_TW = 32, WT_PPT = 2;      // 16 x 32 tile of 4 x 16 patches, two pixels per thread

template <int WH = WT_WH, int WW = WT_WW, int TW_ = WT_TW, int PPT_ = WT_PPT>
struct Tile3 {
    static_assert(WH * WW == 64 && TW_ % WW == 0 && (4 * PPT_) % (TW_ / WW) == 0, "patch / tile shapes");
    static constexpr int TW = TW_, PPT = PPT_;
    static constexpr int PPR = TW / WW;                 // patches per tile row
    static constexpr int TH = WH * (4 * PPT) / PPR;
    int n, ty0, tx0;                                    // sample and tile origin
    int wave, lane;

#ifdef __HIPCC__
    // grid: tiles_x * tiles_y * B workgroups, one dimension
    __device__ __forceinline__ Tile3(int tiles_x, int tiles_y, bool remap = true)
    {
        unsigned bx = blockIdx.x, by, bz;
        if (remap) xcd_remap_calc(gridDim.x, 1, 1, blockIdx.x, bx, by, bz);
        const int tpi = tiles_x * tiles_y;
        n = (int)bx / tpi;
        const int trem = (int)bx - n * tpi;
        ty0 = (trem / tiles_x) * TH; tx0 = (trem - (trem / tiles_x) * tiles_x) * TW;
        wave = threadIdx.x >> 6; lane = threadIdx.x & 63;
    }
    // the workgroup moved to tile t (row-major) of a sample: kernels whose workgroups walk several tiles
    __device__ __forceinline__ void seat(int sample, int t, int tiles_x) { n = sample; ty0 = (t / tiles_x) * TH; tx0 = (t - (t / tiles_x) * tiles_x) * TW; }
    // pass j of this thread: row / column inside the tile, output pixel, pixel offset in the staging tile
    __device__ __forceinline__ int row(int j) const { return ((j * 4 + wave) / PPR) * WH + lane / WW; }
    __device__ __forceinline__ int col(int j) const { return ((j * 4 + wave) % PPR) * WW + lane % WW; }
    __device__ __forceinline__ int y(int j) const { return ty0 + row(j); }
    __device__ __forceinline__ int x(int j) const { return tx0 + col(j); }
    __device__ __forceinline__ int staged(int j) const { return row(j) * TW + col(j); }
    // the prologue of pass j on an OH x OW output: its pixel (yy, xx); false = the pass is parked (never stored) at PARK
    template <Park PARK>
    __device__ __forceinline__ bool pixel(int j, int OH, int OW, int &yy, int &xx) const
    {
        if (PARK == Park::CLAMP) {
            const bool ok = y(j) < OH && x(j) < OW;
            yy = min(y(j), OH - 1); xx = min(x(j), OW - 1);
            return ok;
        }
        yy = y(j); xx = x(j);
        const bool ok = yy < OH && xx < OW;
        if (!ok) { yy = PARK == Park::TILE ? ty0 : 0; xx = PARK == Park::TILE ? tx0 : 0; }
        return ok;
    }

    // The tile, staged in LDS as TH rows of TW pixels of C elements of type E, to out [B, OH, OW, C]: vectors of four elements (a
    // row is TW*C*sizeof(E) bytes from an address the host found aligned to the vector, OW*C % 4 == 0), single elements at a
    // ragged right edge; `vec` false (a run-time choice of the 8-bit kernels) stores single elements throughout.
    template <int C, bool NT = false, typename E>
    __device__ __forceinline__ void store_rows(const E *stage, E *out, int OH, int OW, bool vec = true) const
    {
        typedef E vec4 __attribute__((ext_vector_type(4)));
        __syncthreads();
        const int p0 = (n * OH + ty0) * OW + tx0;           // pixel index of the tile origin: B OH OW < 2^31 (host)
        const int vw = min(TW, OW - tx0) * C;
        if (vec) {
            constexpr int R4 = TW * C / 4;
            for (int e = threadIdx.x; e < TH * R4; e += 256) {
                const int r = e / R4, c4 = e - r * R4;
                if (ty0 + r >= OH || c4 * 4 >= vw) continue;
                E *o = out + (long long)(p0 + r * OW) * C + c4 * 4;
                const vec4 v = *reinterpret_cast<const vec4 *>(stage + r * TW * C + c4 * 4);
                if (c4 * 4 + 4 <= vw) { if (NT) __builtin_nontemporal_store(v, reinterpret_cast<vec4 *>(o)); else *reinterpret_cast<vec4 *>(o) = v; }
                else for (int i = 0; c4 * 4 + i < vw; ++i) o[i] = v[i];
            }
        } else {
            for (int e = threadIdx.x; e < TH * TW * C; e += 256) {
                const int r = e / (TW * C), c = e - r * (TW * C);
                if (ty0 + r < OH && c < vw) out[(long long)(p0 + r * OW) * C + c] = stage[e];
            }
        }
    }
#endif

    // ---- host side
    // tile counts and the one-dimensional grid of a [B, oh, ow] output; false when the grid, or `elems` (the largest element
    // count a kernel indexes with 32 bits: no less than the B oh ow pixels store_rows counts), reaches 2^31
    static bool plan(int B, int oh, int ow, long long elems, int &tx, int &ty, dim3 &grid)
    {
        tx = (ow + TW - 1) / TW; ty = (oh + TH - 1) / TH;
        const long long tiles = (long long)tx * ty * B;
        grid = dim3((unsigned)tiles);
        return tiles < (1ll << 31) && elems < (1ll << 31);
    }
    // the staged instantiation's 16-byte row stores need rows of whole float4s from an aligned base
    static bool staged_ok(const void *out, int ow, int C) { return ((ow * C) & 3) == 0 && ((uintptr_t)out & 15) == 0; }
};

}  // namespace vstab
