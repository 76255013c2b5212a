// The 3-D samplers of the reference's spatial_transformer.py: AffineVolumeTransformer.transform (ST:227-308), bilinear_interp3d
// (ST:797-899) and _meshgrid3d (ST:725-753), forward and backward.  vol [B,D,H,W,C] fp32, one thread per output voxel, any channel
// count.  The per-axis arithmetic is st_axis (st_axis.h), shared with the 2-D family; st3_coords / st3_taps / st3_blend state the
// rest once, and the backward calls the same functions, so its tap decisions are the forward's.
//
// Skeleton: a workgroup owns a BZ x BY x BX BRICK of ONE sample's output and a wave instruction a PZ x PY x PX patch of it, compact
// along all three axes, so that under a rotation the eight gathers of a patch touch a compact set of lines (the 2-D tile study in
// profiles/README.md, one dimension up).  x is the fastest lane index: for C == 1 a brick row leaves as one contiguous run.
// Bricks are numbered through the XCD map (x fastest, then y, z, sample): one XCD's L2 sees a contiguous range of them.  Element
// offsets are 64-bit throughout.  -ffp-contract=off keeps every product and sum its own fp32 operation.
#include "vstab_internal.h"
#include "hbm_profile.h"
#include "st_axis.h"
#include "../../../include/vstab.h"

namespace vstab {

constexpr int BZ = VSTAB_ST3D_BRICK_Z, BY = VSTAB_ST3D_BRICK_Y, BX = VSTAB_ST3D_BRICK_X;
// the wave's patch: as wide in x as the brick up to 16 lanes, two slices deep when the brick has them
#ifndef ST3D_PATCH_X
#define ST3D_PATCH_X (BX < 16 ? BX : 16)
#endif
#ifndef ST3D_PATCH_Z
#define ST3D_PATCH_Z (BZ < 2 ? BZ : 2)
#endif
constexpr int PX = ST3D_PATCH_X, PZ = ST3D_PATCH_Z, PY = 64 / (PX * PZ);
constexpr int WX = BX / PX, WY = BY / PY, WZ = BZ / PZ;                // waves along each axis of the brick
static_assert(PX * PY * PZ == 64 && BX % PX == 0 && BY % PY == 0 && BZ % PZ == 0 && WX * WY * WZ == 4, "brick / patch shapes");

enum { X3_THETA = 0, X3_COORDS = 1 };

struct St3Src {
    const float *x, *y, *z;        // X3_COORDS: flat [B*od*oh*ow]
    const float *theta;            // X3_THETA: [B,12] = row-major 3x4
    int od, oh, ow;                // the output (and linspace grid) size
    float sx, sy, sz;              // the grid's steps 2/(n-1), divided once on the host
    int e;                         // edge_size: voxels of zero pad the coordinates may reach
    int nbx, nby, nbz;             // bricks along each axis
};

// this thread's output voxel: sample n, brick `wg` of that sample, voxel (z, y, x); ok: inside the output
struct Brick {
    int n, wg, z, y, x;
    bool ok;
    __device__ __forceinline__ Brick(const St3Src &S)
    {
        unsigned lin, by_, bz_;
        xcd_remap_calc(gridDim.x, 1, 1, blockIdx.x, lin, by_, bz_);
        const unsigned per = (unsigned)S.nbx * S.nby * S.nbz;          // bricks of one sample; per * B < 2^31 (host)
        n = (int)(lin / per);
        wg = (int)(lin - (unsigned)n * per);
        const int bz = wg / (S.nbx * S.nby), r = wg - bz * (S.nbx * S.nby), by = r / S.nbx, bx = r - by * S.nbx;
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        x = bx * BX + (wave % WX) * PX + lane % PX;
        y = by * BY + ((wave / WX) % WY) * PY + (lane / PX) % PY;
        z = bz * BZ + (wave / (WX * WY)) * PZ + lane / (PX * PY);
        ok = z < S.od && y < S.oh && x < S.ow;
    }
    __device__ __forceinline__ long long voxel(const St3Src &S) const { return (((long long)n * S.od + z) * S.oh + y) * S.ow + x; }
};

// normalised source coordinates of the voxel: explicit, or theta . (x_t, y_t, z_t, 1) with ((t0 x + t1 y) + t2 z) + t3 per row
template <int SRC>
__device__ __forceinline__ void st3_coords(const St3Src &S, const Brick &b, const float *th, float &xt, float &yt, float &zt, float &xs, float &ys, float &zs)
{
    if (SRC == X3_COORDS) {
        const long long i = b.voxel(S);
        xs = S.x[i]; ys = S.y[i]; zs = S.z[i];
        xt = yt = zt = 0.0f;
        return;
    }
    xt = st_grid_t(b.x, S.sx); yt = st_grid_t(b.y, S.sy); zt = st_grid_t(b.z, S.sz);
    xs = ((th[0] * xt + th[1] * yt) + th[2] * zt) + th[3];
    ys = ((th[4] * xt + th[5] * yt) + th[6] * zt) + th[7];
    zs = ((th[8] * xt + th[9] * yt) + th[10] * zt) + th[11];
}

// the eight taps of a voxel, k = 4 zbit + 2 ybit + xbit (bit 1: the v1 tap; ST:859-888's order 000, 001, ..., 111): voxel offset
// inside the sample (clamped into the volume: what is addressed), whether the tap counts (on the zero pad it reads as zero), and the
// weight (wz * wy) * wx
struct Taps3 { long long off[8]; bool valid[8]; float w[8]; };

__device__ __forceinline__ Taps3 st3_taps(const Axis &X, const Axis &Y, const Axis &Z, int H, int W)
{
    Taps3 t;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const bool bz = k & 4, by = k & 2, bx = k & 1;
        t.off[k] = ((long long)(bz ? Z.b : Z.a) * H + (by ? Y.b : Y.a)) * W + (bx ? X.b : X.a);
        t.valid[k] = (bz ? Z.vb : Z.va) && (by ? Y.vb : Y.va) && (bx ? X.vb : X.va);
        t.w[k] = ((bz ? Z.lo : Z.hi) * (by ? Y.lo : Y.hi)) * (bx ? X.lo : X.hi);
    }
    return t;
}

// channel c of the eight taps, a tap on the pad as zero
__device__ __forceinline__ void st3_gather(const Taps3 &t, const float *__restrict__ v, int C, int c, float *I)
{
#pragma unroll
    for (int k = 0; k < 8; ++k) I[k] = t.valid[k] ? v[t.off[k] * C + c] : 0.0f;
}

// tf.add_n of the eight products, left to right (ST:890-898)
__device__ __forceinline__ float st3_blend(const Taps3 &t, const float *I)
{
    float r = t.w[0] * I[0];
#pragma unroll
    for (int k = 1; k < 8; ++k) r = r + t.w[k] * I[k];
    return r;
}

template <int SRC>
__global__ __launch_bounds__(256) void st3d_kernel(const float *__restrict__ vol, int D, int H, int W, int C, St3Src S, float *__restrict__ out)
{
    const Brick b(S);
    if (!b.ok) return;
    float th[12] = {};
    if (SRC == X3_THETA)
#pragma unroll
        for (int k = 0; k < 12; ++k) th[k] = S.theta[(long long)b.n * 12 + k];          // wave-uniform: scalar loads
    float xt, yt, zt, xs, ys, zs;
    st3_coords<SRC>(S, b, th, xt, yt, zt, xs, ys, zs);
    const Taps3 t = st3_taps(st_axis(xs, W, S.e), st_axis(ys, H, S.e), st_axis(zs, D, S.e), H, W);
    const float *__restrict__ v = vol + (long long)b.n * D * H * W * C;
    float *__restrict__ o = out + b.voxel(S) * C;
    for (int c = 0; c < C; ++c) {
        float I[8];
        st3_gather(t, v, C, c, I);
        o[c] = st3_blend(t, I);
    }
}

// _meshgrid3d: flat [4*od*oh*ow] = x_t row, y_t row, z_t row, ones; x fastest, z slowest
__global__ __launch_bounds__(256) void st3d_meshgrid_kernel(float *__restrict__ out, int od, int oh, int ow)
{
    const long long nv = (long long)od * oh * ow, idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= nv) return;
    const long long zy = idx / ow;
    const int ox = (int)(idx - zy * ow), oz = (int)(zy / oh), oy = (int)(zy - (long long)oz * oh);
    out[idx] = lin11(ox, ow);
    out[nv + idx] = lin11(oy, oh);
    out[2 * nv + idx] = lin11(oz, od);
    out[3 * nv + idx] = 1.0f;
}

// ---------------------------------------------------------------------------------
// Backward: what TensorFlow's autodiff gives for ST:797-899 and ST:291-308 (floor and the casts have zero derivative).
//   d vol    the adjoint of the gather: w_k * dout added to the eight taps (none to a tap on the pad) by float atomics -- eight global
//            atomics per voxel-channel; the result DEPENDS ON ATOMIC ARRIVAL ORDER IN ITS LAST BITS.
//   d x/y/z  per voxel: the slope of the trilinear blend along the axis from the eight re-gathered taps (st3_slope, padded-voxel
//            units) times dout, summed over the channels, passed by the clip where -e <= v <= n-1+e inclusive (0 for NaN), times
//            (n - 1) / 2 (st_axis_chain).  Stored for explicit coordinates.
//   d theta  row r of the 3x4 gets g_r * (x_t, y_t, z_t, 1): the products and the sum over voxels in double -- per thread, per wave,
//            per workgroup into part[brick][12], then st_theta_final_kernel<12> in a fixed order: bit-reproducible, no atomics.
// ---------------------------------------------------------------------------------
// one channel's share of d out / d (x, y, z) times its dout g: along x the four differences I[..1] - I[..0], each weighted by its
// (z, y) pair weight, summed in tap order; likewise along y and z
__device__ __forceinline__ void st3_slope(const Axis &X, const Axis &Y, const Axis &Z, const float *I, float g, float &gx, float &gy, float &gz)
{
    gx = gx + ((((I[1] - I[0]) * (Z.hi * Y.hi) + (I[3] - I[2]) * (Z.hi * Y.lo)) + (I[5] - I[4]) * (Z.lo * Y.hi)) + (I[7] - I[6]) * (Z.lo * Y.lo)) * g;
    gy = gy + ((((I[2] - I[0]) * (Z.hi * X.hi) + (I[3] - I[1]) * (Z.hi * X.lo)) + (I[6] - I[4]) * (Z.lo * X.hi)) + (I[7] - I[5]) * (Z.lo * X.lo)) * g;
    gz = gz + ((((I[4] - I[0]) * (Y.hi * X.hi) + (I[5] - I[1]) * (Y.hi * X.lo)) + (I[6] - I[2]) * (Y.lo * X.hi)) + (I[7] - I[3]) * (Y.lo * X.lo)) * g;
}

struct St3Bwd {
    const float *dout;             // [B, od, oh, ow, C]
    float *d_vol;                  // [B, D, H, W, C], added to (null: not wanted)
    float *d_x, *d_y, *d_z;        // X3_COORDS [B*od*oh*ow] (each nullable)
    double *part;                  // X3_THETA [B * bricks][12] (null: d theta not wanted)
};

template <int SRC, bool DVOL, bool DCOORD>
__global__ __launch_bounds__(256) void st3d_bwd_kernel(const float *__restrict__ vol, int D, int H, int W, int C, St3Src S, St3Bwd G)
{
    __shared__ double red[4][12];
    const Brick b(S);
    double acc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (b.ok) {
        float th[12] = {};
        if (SRC == X3_THETA)
#pragma unroll
            for (int k = 0; k < 12; ++k) th[k] = S.theta[(long long)b.n * 12 + k];
        float xt, yt, zt, xs, ys, zs;
        st3_coords<SRC>(S, b, th, xt, yt, zt, xs, ys, zs);
        const Axis X = st_axis(xs, W, S.e), Y = st_axis(ys, H, S.e), Z = st_axis(zs, D, S.e);
        const Taps3 t = st3_taps(X, Y, Z, H, W);
        const long long vox = b.voxel(S);
        const float *__restrict__ v = vol + (long long)b.n * D * H * W * C;
        const float *__restrict__ g = G.dout + vox * C;
        float *dv = DVOL ? G.d_vol + (long long)b.n * D * H * W * C : nullptr;
        float gx = 0.f, gy = 0.f, gz = 0.f;
        for (int c = 0; c < C; ++c) {
            const float gc = g[c];
            if (DCOORD) {
                float I[8];
                st3_gather(t, v, C, c, I);
                st3_slope(X, Y, Z, I, gc, gx, gy, gz);
            }
            if (DVOL) {
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    if (t.valid[k]) atomicAdd(dv + t.off[k] * C + c, t.w[k] * gc);
            }
        }
        if (DCOORD) {
            const float gxn = st_axis_chain(X, gx, W), gyn = st_axis_chain(Y, gy, H), gzn = st_axis_chain(Z, gz, D);
            if (SRC == X3_COORDS) {
                if (G.d_x) G.d_x[vox] = gxn;
                if (G.d_y) G.d_y[vox] = gyn;
                if (G.d_z) G.d_z[vox] = gzn;
            } else {
                const double gr[3] = {(double)gxn, (double)gyn, (double)gzn};
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    acc[4 * r] += gr[r] * (double)xt; acc[4 * r + 1] += gr[r] * (double)yt;
                    acc[4 * r + 2] += gr[r] * (double)zt; acc[4 * r + 3] += gr[r];
                }
            }
        }
    }
    if (DCOORD && SRC == X3_THETA) {
        const long long per = (long long)S.nbx * S.nby * S.nbz;
        st_theta_reduce<12>(acc, red, G.part + ((long long)b.n * per + b.wg) * 12);
    }
}

// ---- host side
// bricks along each axis and per sample; false when the one-dimensional grid of B samples does not fit 31 bits
bool st3d_plan(int B, int od, int oh, int ow, int &nbx, int &nby, int &nbz, long long &bricks)
{
    nbx = (ow + BX - 1) / BX; nby = (oh + BY - 1) / BY; nbz = (od + BZ - 1) / BZ;
    bricks = (long long)nbx * nby * nbz;               // each factor < 2^24 (api.cpp): the product of two fits 63 bits ...
    if ((long long)nbx * nby >= (1ll << 31) || bricks >= (1ll << 31)) return false;      // ... and is checked before the third
    return bricks * B < (1ll << 31);
}

static St3Src st3d_src(int B, int od, int oh, int ow, int e)
{
    St3Src S{};
    S.od = od; S.oh = oh; S.ow = ow; S.e = e;
    S.sx = ow > 1 ? 2.0f / (float)(ow - 1) : 0.0f; S.sy = oh > 1 ? 2.0f / (float)(oh - 1) : 0.0f; S.sz = od > 1 ? 2.0f / (float)(od - 1) : 0.0f;
    long long bricks;
    st3d_plan(B, od, oh, ow, S.nbx, S.nby, S.nbz, bricks);
    return S;
}

static dim3 st3d_grid(const St3Src &S, int B) { return dim3((unsigned)((long long)S.nbx * S.nby * S.nbz * B)); }

hipError_t launch_st3d_meshgrid(float *out, int od, int oh, int ow, hipStream_t stream)
{
    const long long nv = (long long)od * oh * ow;
    st3d_meshgrid_kernel<<<dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, stream>>>(out, od, oh, ow);
    return hipGetLastError();
}

hipError_t launch_st3d_interp(const float *vol, int B, int D, int H, int W, int C, const float *x, const float *y, const float *z, int od, int oh,
                              int ow, int edge, float *out, hipStream_t stream)
{
    St3Src S = st3d_src(B, od, oh, ow, edge);
    S.x = x; S.y = y; S.z = z;
    return launch_timed(-1, 0.0, st3d_kernel<X3_COORDS>, st3d_grid(S, B), dim3(256), stream, vol, D, H, W, C, S, out);
}

hipError_t launch_st3d_transform(const float *vol, int B, int D, int H, int W, int C, const float *theta, float *out, int od, int oh, int ow,
                                 hipStream_t stream)
{
    St3Src S = st3d_src(B, od, oh, ow, 1);
    S.theta = theta;
    return launch_timed(-1, 0.0, st3d_kernel<X3_THETA>, st3d_grid(S, B), dim3(256), stream, vol, D, H, W, C, S, out);
}

size_t st3d_transform_backward_ws_bytes(int B, int od, int oh, int ow)
{
    int nbx, nby, nbz;
    long long bricks;
    if (!st3d_plan(B, od, oh, ow, nbx, nby, nbz, bricks)) return 0;
    return (size_t)bricks * B * 12 * sizeof(double);
}

template <int SRC>
static hipError_t launch_st3d_bwd(const float *vol, int B, int D, int H, int W, int C, const St3Src &S, const St3Bwd &G, int accumulate, hipStream_t stream)
{
    if (G.d_vol && !accumulate) {
        const hipError_t e = hipMemsetAsync(G.d_vol, 0, (size_t)B * D * H * W * C * sizeof(float), stream);
        if (e != hipSuccess) return e;
    }
    const bool dvol = G.d_vol != nullptr, dcoord = SRC == X3_THETA ? G.part != nullptr : (G.d_x || G.d_y || G.d_z);
    const dim3 grid = st3d_grid(S, B);
#define ST3D_BWD(V, K) st3d_bwd_kernel<SRC, V, K><<<grid, dim3(256), 0, stream>>>(vol, D, H, W, C, S, G)
    if (dvol && dcoord) ST3D_BWD(true, true);
    else if (dvol) ST3D_BWD(true, false);
    else ST3D_BWD(false, true);
#undef ST3D_BWD
    return hipGetLastError();
}

hipError_t launch_st3d_transform_backward(const float *vol, int B, int D, int H, int W, int C, const float *theta, const float *dout, int od, int oh,
                                          int ow, float *d_vol, int accumulate, float *d_theta, double *part, hipStream_t stream)
{
    St3Src S = st3d_src(B, od, oh, ow, 1);
    S.theta = theta;
    const St3Bwd G{dout, d_vol, nullptr, nullptr, nullptr, d_theta ? part : nullptr};
    const hipError_t e = launch_st3d_bwd<X3_THETA>(vol, B, D, H, W, C, S, G, accumulate, stream);
    if (e != hipSuccess || !d_theta) return e;
    st_theta_final_kernel<12><<<dim3((unsigned)B), dim3(256), 0, stream>>>(part, S.nbx * S.nby * S.nbz, 12, d_theta);
    return hipGetLastError();
}

hipError_t launch_st3d_interp_backward(const float *vol, int B, int D, int H, int W, int C, const float *x, const float *y, const float *z,
                                       int od, int oh, int ow, int edge, const float *dout, float *d_vol, int accumulate, float *d_x, float *d_y,
                                       float *d_z, hipStream_t stream)
{
    St3Src S = st3d_src(B, od, oh, ow, edge);
    S.x = x; S.y = y; S.z = z;
    const St3Bwd G{dout, d_vol, d_x, d_y, d_z, nullptr};
    return launch_st3d_bwd<X3_COORDS>(vol, B, D, H, W, C, S, G, accumulate, stream);
}

}  // namespace vstab
