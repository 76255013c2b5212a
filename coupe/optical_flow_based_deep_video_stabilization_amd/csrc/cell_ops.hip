// Kernels of cell.py's recurrent cells (cell.py:5-136): everything a ConvLSTMCell / ConvGRUCell step does AFTER its SAME convolution
// (which runs on conv_mfma.hip through vstab_conv_forward) -- gate split, peephole products, tf.contrib.layers.layer_norm of each
// gate, sigmoid / activation and the state update.  Forward only.
//
// Index space: one sample's gate is N = H*W*F numbers, element e = pixel * F + channel; y is the convolution's output
// [B, H*W, ys] with gate g in channels g*F .. g*F+F-1 (ys >= the number of gate channels: the rows may be padded).  Every kernel runs
// on a grid (ceil(N / CHUNK), B) of 256 threads; a workgroup owns CHUNK = 2048 consecutive elements of one sample, 8 per thread at a
// stride of 256 (consecutive lanes read consecutive floats).
//
// Layer norm (ln_apply below, the one place that states it): per sample, mean and BIASED variance over all N numbers of the gate,
//   out = (v - mean) * rsqrt(var + 1e-12) * gamma[ch] + beta[ch].
// Statistics: a workgroup holds its chunk in registers, sums it (double across the workgroup), takes the rounded chunk mean as a
// shift s and sums (v - s)^2 -- mean first, then the centred second moment, of numbers that never left the registers.  It stores
// {sum, s, sum (v-s)^2} as three doubles; cell_stats_kernel (one wave per sample and gate) combines the chunks in a fixed order in
// double with the pairwise update M2 += M2_k + n_k (mean_k - mean)^2 and writes {mean, rstd} as floats.  No atomics anywhere:
// two runs give the same bits, and a sample's numbers depend on nothing but that sample.
#include "vstab_internal.h"

namespace vstab {

namespace {

constexpr int CELL_E = CELL_CHUNK / 256;            // elements per thread

template <int ACT> __device__ __forceinline__ float cell_act(float v)
{
    if (ACT == 0) return tanhf(v);
    if (ACT == 1) return v > 0.f ? v : 0.f;
    return v;
}

__device__ __forceinline__ float cell_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }

// tf.contrib.layers.layer_norm's arithmetic on one number, given the sample's statistics
__device__ __forceinline__ float ln_apply(float v, float2 mean_rstd, float gamma, float beta)
{
    return (v - mean_rstd.x) * mean_rstd.y * gamma + beta;
}

// sums of Q doubles over the 256 threads in a fixed order; every thread gets the result.  red: Q * 4 doubles
template <int Q> __device__ __forceinline__ void block_sum(double (&v)[Q], double *red)
{
#pragma unroll
    for (int q = 0; q < Q; ++q)
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v[q] += __shfl_xor(v[q], off, 64);
    __syncthreads();                                 // (red may still be read from the previous call)
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int q = 0; q < Q; ++q) red[q * 4 + (threadIdx.x >> 6)] = v[q];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < Q; ++q) v[q] = (red[q * 4] + red[q * 4 + 1]) + (red[q * 4 + 2] + red[q * 4 + 3]);
}

// the chunk's {sum, shift, sum of (v - shift)^2} of Q quantities held as val[q][it] (entries with !ok[it] are ignored), stored to
// partial[((b * Q + q) * nchunk + chunk) * 3 ..]
template <int Q>
__device__ __forceinline__ void chunk_moments(const float (&val)[Q][CELL_E], const bool (&ok)[CELL_E], int n_chunk, double *__restrict__ partial,
                                              double *red)
{
    double s[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        float a = 0.f;
#pragma unroll
        for (int it = 0; it < CELL_E; ++it) a += ok[it] ? val[q][it] : 0.f;
        s[q] = (double)a;
    }
    block_sum<Q>(s, red);
    float shift[Q];
    double m2[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        shift[q] = (float)(s[q] / (double)n_chunk);
        float a = 0.f;
#pragma unroll
        for (int it = 0; it < CELL_E; ++it) {
            const float d = val[q][it] - shift[q];
            a += ok[it] ? d * d : 0.f;
        }
        m2[q] = (double)a;
    }
    block_sum<Q>(m2, red);
    if (threadIdx.x == 0) {
        const size_t nchunk = gridDim.x;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            double *p = partial + (((size_t)blockIdx.y * Q + q) * nchunk + blockIdx.x) * 3;
            p[0] = s[q]; p[1] = (double)shift[q]; p[2] = m2[q];
        }
    }
}

// grid (Q, B), one wave: stats[b * Q + q] = {mean, 1 / sqrt(var + 1e-12)} of the N numbers whose chunk moments are in partial
__global__ __launch_bounds__(64) void cell_stats_kernel(const double *__restrict__ partial, int nchunk, int N, float2 *__restrict__ stats)
{
    const int q = blockIdx.x, Q = gridDim.x, b = blockIdx.y, lane = threadIdx.x;
    const double *p = partial + ((size_t)b * Q + q) * nchunk * 3;
    double sum = 0.0;
    for (int k = lane; k < nchunk; k += 64) sum += p[(size_t)k * 3];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off, 64);
    const double mean = sum / (double)N;
    double m2 = 0.0;
    for (int k = lane; k < nchunk; k += 64) {
        const double nk = (double)min(CELL_CHUNK, N - k * CELL_CHUNK);
        const double mk = p[(size_t)k * 3] / nk, sk = p[(size_t)k * 3 + 1];
        // sum (v - mk)^2 = sum (v - sk)^2 - nk (mk - sk)^2, then the shift from the chunk's mean to the sample's
        m2 += p[(size_t)k * 3 + 2] - nk * (mk - sk) * (mk - sk) + nk * (mk - mean) * (mk - mean);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m2 += __shfl_xor(m2, off, 64);
    if (lane == 0) {
        const double var = fmax(m2, 0.0) / (double)N;
        stats[b * Q + q] = make_float2((float)mean, (float)(1.0 / sqrt(var + 1e-12)));
    }
}

// what a thread needs to address its CELL_E elements
struct CellIdx {
    // (32-bit: the API admits no tensor of 2^31 elements or more, strided ones included)
    unsigned yoff[CELL_E];      // pixel's offset in a [B, HW, stride] tensor, in units of the stride (= b * HW + pixel)
    unsigned eoff[CELL_E];      // element's offset in a contiguous [B, N] tensor
    int ch[CELL_E], e[CELL_E];
    bool ok[CELL_E];
    int n_chunk;
};

__device__ __forceinline__ void cell_index(int HW, int F, CellIdx &ix)
{
    const int N = HW * F, b = blockIdx.y, e0 = blockIdx.x * CELL_CHUNK;
    ix.n_chunk = min(CELL_CHUNK, N - e0);
#pragma unroll
    for (int it = 0; it < CELL_E; ++it) {
        const int e = e0 + it * 256 + (int)threadIdx.x;
        ix.ok[it] = e < N;
        const int ee = ix.ok[it] ? e : 0;             // (an index that exists: nothing is read or written through it when !ok)
        const int px = ee / F;
        ix.e[it] = ee;
        ix.ch[it] = ee - px * F;
        ix.yoff[it] = (unsigned)b * HW + px;
        ix.eoff[it] = (unsigned)b * N + ee;
    }
}

// ---------------------------------------------------------------------------------------------------------------- ConvLSTM
struct LstmArgs {
    const float *y; int ys;                       // [B, HW, ys]: j, i, f, o at channels 0, F, 2F, 3F
    const float *c;                               // [B, N] old state
    const float *wci, *wcf, *wco;                 // [N] peepholes
    const float *gamma, *beta;                    // [5][F]: j, i, f, o, c
    int HW, F;
    float forget_bias;
    const float2 *stats_a, *stats_b;              // [B][3], [B][2]
    double *part_a, *part_b;
    float *o_tmp, *c_tmp;                         // [B, N] (normalize only)
    float *c_out, *h_out;                         // [B, N]
    float *h_cat; int cs_cat;                     // the h slice of the concat buffer: first channel of pixel 0, pixel stride
};

template <bool PEEP>
__device__ __forceinline__ void lstm_load_jif(const LstmArgs &a, const CellIdx &ix, float (&v)[3][CELL_E], float (&cold)[CELL_E])
{
#pragma unroll
    for (int it = 0; it < CELL_E; ++it) {
        v[0][it] = v[1][it] = v[2][it] = cold[it] = 0.f;
        if (!ix.ok[it]) continue;
        const float *yp = a.y + ix.yoff[it] * a.ys + ix.ch[it];
        cold[it] = a.c[ix.eoff[it]];
        v[0][it] = yp[0];
        v[1][it] = yp[a.F];
        v[2][it] = yp[2 * a.F];
        if (PEEP) {
            v[1][it] += a.wci[ix.e[it]] * cold[it];
            v[2][it] += a.wcf[ix.e[it]] * cold[it];
        }
    }
}

// A: chunk moments of j, i + W_ci c, f + W_cf c
template <bool PEEP> __global__ __launch_bounds__(256) void lstm_a_kernel(LstmArgs a)
{
    __shared__ double red[12];
    CellIdx ix;
    cell_index(a.HW, a.F, ix);
    float v[3][CELL_E], cold[CELL_E];
    lstm_load_jif<PEEP>(a, ix, v, cold);
    chunk_moments<3>(v, ix.ok, ix.n_chunk, a.part_a, red);
}

// B: c' = c f + i act(j) and o + W_co c'.  NORM: both stored for C with their chunk moments; otherwise h' at once
template <bool NORM, bool PEEP, int ACT> __global__ __launch_bounds__(256) void lstm_b_kernel(LstmArgs a)
{
    __shared__ double red[8];
    CellIdx ix;
    cell_index(a.HW, a.F, ix);
    float v[3][CELL_E], cold[CELL_E], oc[2][CELL_E];
    lstm_load_jif<PEEP>(a, ix, v, cold);
    float2 st[3];
    if (NORM)
#pragma unroll
        for (int q = 0; q < 3; ++q) st[q] = a.stats_a[blockIdx.y * 3 + q];
#pragma unroll
    for (int it = 0; it < CELL_E; ++it) {
        oc[0][it] = oc[1][it] = 0.f;
        if (!ix.ok[it]) continue;
        const int ch = ix.ch[it];
        float j = v[0][it], i = v[1][it], f = v[2][it];
        if (NORM) {
            j = ln_apply(j, st[0], a.gamma[ch], a.beta[ch]);
            i = ln_apply(i, st[1], a.gamma[a.F + ch], a.beta[a.F + ch]);
            f = ln_apply(f, st[2], a.gamma[2 * a.F + ch], a.beta[2 * a.F + ch]);
        }
        f = cell_sigmoid(f + a.forget_bias);
        i = cell_sigmoid(i);
        const float cn = cold[it] * f + i * cell_act<ACT>(j);
        float o = a.y[ix.yoff[it] * a.ys + 3 * a.F + ch];
        if (PEEP) o += a.wco[ix.e[it]] * cn;
        if (NORM) {
            oc[0][it] = o; oc[1][it] = cn;
            a.o_tmp[ix.eoff[it]] = o;
            a.c_tmp[ix.eoff[it]] = cn;
        } else {
            const float h = cell_sigmoid(o) * cell_act<ACT>(cn);
            a.c_out[ix.eoff[it]] = cn;
            a.h_out[ix.eoff[it]] = h;
            if (a.h_cat) a.h_cat[ix.yoff[it] * a.cs_cat + ch] = h;
        }
    }
    if (NORM) chunk_moments<2>(oc, ix.ok, ix.n_chunk, a.part_b, red);
}

// C: o = LN(o), c' = LN(c'), h' = sigmoid(o) act(c')
template <int ACT> __global__ __launch_bounds__(256) void lstm_c_kernel(LstmArgs a)
{
    CellIdx ix;
    cell_index(a.HW, a.F, ix);
    const float2 so = a.stats_b[blockIdx.y * 2], sc = a.stats_b[blockIdx.y * 2 + 1];
#pragma unroll
    for (int it = 0; it < CELL_E; ++it) {
        if (!ix.ok[it]) continue;
        const int ch = ix.ch[it];
        const float o = ln_apply(a.o_tmp[ix.eoff[it]], so, a.gamma[3 * a.F + ch], a.beta[3 * a.F + ch]);
        const float cn = ln_apply(a.c_tmp[ix.eoff[it]], sc, a.gamma[4 * a.F + ch], a.beta[4 * a.F + ch]);
        const float h = cell_sigmoid(o) * cell_act<ACT>(cn);
        a.c_out[ix.eoff[it]] = cn;
        a.h_out[ix.eoff[it]] = h;
        if (a.h_cat) a.h_cat[ix.yoff[it] * a.cs_cat + ch] = h;
    }
}

// ---------------------------------------------------------------------------------------------------------------- ConvGRU
struct GruArgs {
    const float *y; int ys;                       // gates: r, u at channels 0, F; update: the candidate at channel 0
    const float *h; int hs;                       // the old state as a slice: first channel of pixel 0, pixel stride
    const float *gamma, *beta;                    // gates [2][F] (r, u); update [F]
    int HW, F;
    const float2 *stats;
    double *part;
    float *rh; int rhs;                           // gates: r h into the candidate buffer's slice
    float *u;                                     // [B, N]: written by gates, read by update
    float *h_out;                                 // update: [B, N]
    float *h_new; int hns;                        // update: the new state as a slice (may be the one h came from)
};

template <int Q> __global__ __launch_bounds__(256) void gru_moments_kernel(GruArgs a)
{
    __shared__ double red[Q * 4];
    CellIdx ix;
    cell_index(a.HW, a.F, ix);
    float v[Q][CELL_E];
#pragma unroll
    for (int it = 0; it < CELL_E; ++it)
#pragma unroll
        for (int q = 0; q < Q; ++q) v[q][it] = ix.ok[it] ? a.y[ix.yoff[it] * a.ys + q * a.F + ix.ch[it]] : 0.f;
    chunk_moments<Q>(v, ix.ok, ix.n_chunk, a.part, red);
}

template <bool NORM> __global__ __launch_bounds__(256) void gru_gates_kernel(GruArgs a)
{
    CellIdx ix;
    cell_index(a.HW, a.F, ix);
    float2 sr = make_float2(0.f, 0.f), su = sr;
    if (NORM) { sr = a.stats[blockIdx.y * 2]; su = a.stats[blockIdx.y * 2 + 1]; }
#pragma unroll
    for (int it = 0; it < CELL_E; ++it) {
        if (!ix.ok[it]) continue;
        const int ch = ix.ch[it];
        const float *yp = a.y + ix.yoff[it] * a.ys + ch;
        float r = yp[0], u = yp[a.F];
        if (NORM) {
            r = ln_apply(r, sr, a.gamma[ch], a.beta[ch]);
            u = ln_apply(u, su, a.gamma[a.F + ch], a.beta[a.F + ch]);
        }
        r = cell_sigmoid(r);
        u = cell_sigmoid(u);
        a.rh[ix.yoff[it] * a.rhs + ch] = r * a.h[ix.yoff[it] * a.hs + ch];
        a.u[ix.eoff[it]] = u;
    }
}

template <bool NORM, int ACT> __global__ __launch_bounds__(256) void gru_update_kernel(GruArgs a)
{
    CellIdx ix;
    cell_index(a.HW, a.F, ix);
    float2 sy = make_float2(0.f, 0.f);
    if (NORM) sy = a.stats[blockIdx.y];
#pragma unroll
    for (int it = 0; it < CELL_E; ++it) {
        if (!ix.ok[it]) continue;
        const int ch = ix.ch[it];
        float y2 = a.y[ix.yoff[it] * a.ys + ch];
        if (NORM) y2 = ln_apply(y2, sy, a.gamma[ch], a.beta[ch]);
        const float u = a.u[ix.eoff[it]], h = a.h[ix.yoff[it] * a.hs + ch];
        const float hn = u * h + (1.0f - u) * cell_act<ACT>(y2);
        a.h_out[ix.eoff[it]] = hn;
        if (a.h_new) a.h_new[ix.yoff[it] * a.hns + ch] = hn;
    }
}

inline dim3 cell_grid(int B, int N) { return dim3((unsigned)cell_chunks(N), (unsigned)B); }

// the workspace of one call, carved the same way by the size function and the launchers
struct CellWs { size_t part_a, part_b, stats_a, stats_b, o_tmp, c_tmp, total; };

inline size_t up256(size_t n) { return (n + 255) / 256 * 256; }

CellWs cell_ws(int B, int N, int qa, int qb, bool tmp)
{
    CellWs w{};
    const size_t nch = (size_t)cell_chunks(N);
    size_t off = 0;
    w.part_a = off; off += up256((size_t)B * qa * nch * 3 * sizeof(double));
    w.part_b = off; off += up256((size_t)B * qb * nch * 3 * sizeof(double));
    w.stats_a = off; off += up256((size_t)B * qa * sizeof(float2));
    w.stats_b = off; off += up256((size_t)B * qb * sizeof(float2));
    w.o_tmp = off; off += tmp ? up256((size_t)B * N * sizeof(float)) : 0;
    w.c_tmp = off; off += tmp ? up256((size_t)B * N * sizeof(float)) : 0;
    w.total = off;
    return w;
}

}  // namespace

int cell_chunks(int N) { return (N + CELL_CHUNK - 1) / CELL_CHUNK; }

size_t convlstm_workspace_bytes(int B, int HW, int F, bool normalize)
{
    return normalize ? cell_ws(B, HW * F, 3, 2, true).total : 0;
}

size_t convgru_workspace_bytes(int B, int HW, int F, bool normalize)
{
    return normalize ? cell_ws(B, HW * F, 2, 0, false).total : 0;
}

#define CELL_FOR_ACT(act, CALL)                  \
    switch (act) {                               \
    case 0: CALL(0); break;                      \
    case 1: CALL(1); break;                      \
    case 2: CALL(2); break;                      \
    default: return hipErrorInvalidValue;        \
    }

hipError_t launch_convlstm_gates(const float *y, int ys, const float *c, const float *wci, const float *wcf, const float *wco, const float *gamma,
                                 const float *beta, int B, int HW, int F, float forget_bias, int act, bool normalize, bool peephole, float *c_out,
                                 float *h_out, float *h_cat, int cs_cat, void *workspace, hipStream_t stream)
{
    const int N = HW * F;
    LstmArgs a{};
    a.y = y; a.ys = ys; a.c = c; a.wci = wci; a.wcf = wcf; a.wco = wco; a.gamma = gamma; a.beta = beta; a.HW = HW; a.F = F;
    a.forget_bias = forget_bias; a.c_out = c_out; a.h_out = h_out; a.h_cat = h_cat; a.cs_cat = cs_cat;
    const dim3 grid = cell_grid(B, N), blk(256);
    if (!normalize) {
#define CALL(A)                                                                          \
    if (peephole) lstm_b_kernel<false, true, A><<<grid, blk, 0, stream>>>(a);            \
    else lstm_b_kernel<false, false, A><<<grid, blk, 0, stream>>>(a)
        CELL_FOR_ACT(act, CALL)
#undef CALL
        return hipGetLastError();
    }
    const CellWs w = cell_ws(B, N, 3, 2, true);
    char *ws = reinterpret_cast<char *>(workspace);
    a.part_a = reinterpret_cast<double *>(ws + w.part_a);
    a.part_b = reinterpret_cast<double *>(ws + w.part_b);
    a.stats_a = reinterpret_cast<const float2 *>(ws + w.stats_a);
    a.stats_b = reinterpret_cast<const float2 *>(ws + w.stats_b);
    a.o_tmp = reinterpret_cast<float *>(ws + w.o_tmp);
    a.c_tmp = reinterpret_cast<float *>(ws + w.c_tmp);
    if (peephole) lstm_a_kernel<true><<<grid, blk, 0, stream>>>(a);
    else lstm_a_kernel<false><<<grid, blk, 0, stream>>>(a);
    cell_stats_kernel<<<dim3(3, (unsigned)B), dim3(64), 0, stream>>>(a.part_a, (int)grid.x, N, reinterpret_cast<float2 *>(ws + w.stats_a));
#define CALL(A)                                                                         \
    if (peephole) lstm_b_kernel<true, true, A><<<grid, blk, 0, stream>>>(a);            \
    else lstm_b_kernel<true, false, A><<<grid, blk, 0, stream>>>(a)
    CELL_FOR_ACT(act, CALL)
#undef CALL
    cell_stats_kernel<<<dim3(2, (unsigned)B), dim3(64), 0, stream>>>(a.part_b, (int)grid.x, N, reinterpret_cast<float2 *>(ws + w.stats_b));
#define CALL(A) lstm_c_kernel<A><<<grid, blk, 0, stream>>>(a)
    CELL_FOR_ACT(act, CALL)
#undef CALL
    return hipGetLastError();
}

hipError_t launch_convgru_gates(const float *y, int ys, const float *h, int hs, const float *gamma, const float *beta, int B, int HW, int F,
                                bool normalize, float *rh, int rhs, float *u, void *workspace, hipStream_t stream)
{
    const int N = HW * F;
    GruArgs a{};
    a.y = y; a.ys = ys; a.h = h; a.hs = hs; a.gamma = gamma; a.beta = beta; a.HW = HW; a.F = F; a.rh = rh; a.rhs = rhs; a.u = u;
    const dim3 grid = cell_grid(B, N), blk(256);
    if (normalize) {
        const CellWs w = cell_ws(B, N, 2, 0, false);
        char *ws = reinterpret_cast<char *>(workspace);
        a.part = reinterpret_cast<double *>(ws + w.part_a);
        a.stats = reinterpret_cast<const float2 *>(ws + w.stats_a);
        gru_moments_kernel<2><<<grid, blk, 0, stream>>>(a);
        cell_stats_kernel<<<dim3(2, (unsigned)B), dim3(64), 0, stream>>>(a.part, (int)grid.x, N, reinterpret_cast<float2 *>(ws + w.stats_a));
        gru_gates_kernel<true><<<grid, blk, 0, stream>>>(a);
    } else {
        gru_gates_kernel<false><<<grid, blk, 0, stream>>>(a);
    }
    return hipGetLastError();
}

hipError_t launch_convgru_update(const float *y2, int ys, const float *h, int hs, const float *u, const float *gamma, const float *beta, int B,
                                 int HW, int F, int act, bool normalize, float *h_out, float *h_new, int hns, void *workspace,
                                 hipStream_t stream)
{
    const int N = HW * F;
    GruArgs a{};
    a.y = y2; a.ys = ys; a.h = h; a.hs = hs; a.gamma = gamma; a.beta = beta; a.HW = HW; a.F = F; a.u = const_cast<float *>(u);
    a.h_out = h_out; a.h_new = h_new; a.hns = hns;
    const dim3 grid = cell_grid(B, N), blk(256);
    if (normalize) {
        const CellWs w = cell_ws(B, N, 2, 0, false);          // (the gates' carving: one workspace serves both calls)
        char *ws = reinterpret_cast<char *>(workspace);
        a.part = reinterpret_cast<double *>(ws + w.part_a);
        a.stats = reinterpret_cast<const float2 *>(ws + w.stats_a);
        gru_moments_kernel<1><<<grid, blk, 0, stream>>>(a);
        cell_stats_kernel<<<dim3(1, (unsigned)B), dim3(64), 0, stream>>>(a.part, (int)grid.x, N, reinterpret_cast<float2 *>(ws + w.stats_a));
#define CALL(A) gru_update_kernel<true, A><<<grid, blk, 0, stream>>>(a)
        CELL_FOR_ACT(act, CALL)
#undef CALL
    } else {
#define CALL(A) gru_update_kernel<false, A><<<grid, blk, 0, stream>>>(a)
        CELL_FOR_ACT(act, CALL)
#undef CALL
    }
    return hipGetLastError();
}

}  // namespace vstab
