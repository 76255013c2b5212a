// Kernels of cell.py's recurrent cells (cell.py:5-136): everything a ConvLSTMCell / ConvGRUCell step does AFTER its SAME convolution
// (which runs on conv_mfma.hip through vstab_conv_forward) -- gate split, peephole products, tf.contrib.layers.layer_norm of each
// gate, sigmoid / activation and the state update -- and, further down, the backward of the same stages.
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
//
// Backward (second half of the file): the same index space and guarantees.  Gate values are recomputed from y, the old state and the
// forward's {mean, rstd} pairs; nothing else is stored.  A layer norm's adjoint (ln_apply_adjoint below) needs two per-sample means
// (of g = dout gamma and of g xhat): a pass writes the gradient with respect to the layer norm's OUTPUT into dy and the chunk sums of
// g and g xhat (double across the workgroup), cell_sums_kernel combines the chunks in a fixed order, and the next pass turns dy
// into the gradient of the layer norm's input in place.  With normalize that is, as in the forward, pass / sums / pass / sums / pass
// for the LSTM (two layer-norm depths) and pass / sums / pass for the GRU stages; without it one pass.  Parameter gradients: the
// per-channel sums of gamma / beta are column sums in double (row-chunk partials, then the chunks in order) of a
// [B*HW, 2*Q*F] table of products that the passes write; the peepholes' per-element sums over the batch are taken sample by
// sample, in double, by one thread per element.  No float atomics: two runs give the same bits, and the input / state gradients of a sample
// depend on that sample only.
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

// its normalised argument xhat (ln_apply = ln_xhat * gamma + beta, the same roundings) ...
__device__ __forceinline__ float ln_xhat(float v, float2 mean_rstd) { return (v - mean_rstd.x) * mean_rstd.y; }

// ... and its adjoint with respect to v, given dout of this number, g = dout * gamma, and the sample's means of g and of g * xhat over
// the N numbers of the gate:  dv = rstd * (g - mean(g) - xhat * mean(g xhat)).  (dgamma[ch] = sum dout xhat and dbeta[ch] = sum dout
// over samples and pixels are the callers' column sums.)
__device__ __forceinline__ float ln_apply_adjoint(float dout, float gamma, float xhat, float rstd, float mean_g, float mean_gx)
{
    return rstd * (dout * gamma - mean_g - xhat * mean_gx);
}

// d act(v) / dv given a = act(v); relu takes the forward's branch
template <int ACT> __device__ __forceinline__ float cell_act_grad(float v, float a)
{
    if (ACT == 0) return 1.0f - a * a;
    if (ACT == 1) return v > 0.f ? 1.0f : 0.f;
    return 1.0f;
}

__device__ __forceinline__ float sigmoid_grad(float s) { return s * (1.0f - s); }

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

// ================================================================================================================ backward
// chunk sums of Q per-thread floats, stored to partial[(b * Q + q) * nchunk + chunk]
template <int Q> __device__ __forceinline__ void chunk_sums(const float (&acc)[Q], double *__restrict__ partial, double *red)
{
    double s[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) s[q] = (double)acc[q];
    block_sum<Q>(s, red);
    if (threadIdx.x == 0)
#pragma unroll
        for (int q = 0; q < Q; ++q) partial[((size_t)blockIdx.y * Q + q) * gridDim.x + blockIdx.x] = s[q];
}

// grid (Q, B), one wave: sums[b * Q + q] = (sum over the chunks, in a fixed order) / N
__global__ __launch_bounds__(64) void cell_sums_kernel(const double *__restrict__ partial, int nchunk, int N, float *__restrict__ sums)
{
    const int q = blockIdx.x, Q = gridDim.x, b = blockIdx.y, lane = threadIdx.x;
    const double *p = partial + ((size_t)b * Q + q) * nchunk;
    double sum = 0.0;
    for (int k = lane; k < nchunk; k += 64) sum += p[k];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off, 64);
    if (lane == 0) sums[b * Q + q] = (float)(sum / (double)N);
}

// the pad channels nch .. stride-1 of a pixel's dy row are written as zero by the thread that owns the pixel's channel 0
__device__ __forceinline__ void zero_pads(float *row, int nch, int stride)
{
    for (int p = nch; p < stride; ++p) row[p] = 0.f;
}

// one row of the gamma / beta product table: [.., q * F + ch] = dout * xhat, [.., (Q + q) * F + ch] = dout
__device__ __forceinline__ void prod_store(float *prod, unsigned yoff, int Q, int F, int q, int ch, float dout, float xhat)
{
    float *row = prod + (size_t)yoff * (2 * Q * F);
    row[q * F + ch] = dout * xhat;
    row[(Q + q) * F + ch] = dout;
}

struct LstmBwdArgs {
    LstmArgs f;                                   // the forward's inputs: y, c, peepholes, gamma, beta, forget_bias, stats_a, stats_b
    const float *dh; int dhs;                     // d h' as a slice (may be NULL: zero)
    const float *dcn;                             // d c' [B, N] (may be NULL: zero)
    float *dy; int dys;                           // [B, HW, dys]: dj, di, df, do
    float *dc;                                    // [B, N]: d c (the old state)
    float *c_raw;                                 // [B, N]: c' before its layer norm, for dW_co (NULL: not wanted)
    float *prod;                                  // [B*HW, 10 F] (NULL: gamma / beta gradients not wanted)
    double *part1, *part2;
    const float *sums1, *sums2;                   // [B][4]: o, c;  [B][6]: j, i, f  ({mean g, mean g xhat} each)
};

// what the forward computed for one element, recomputed
struct LstmEl {
    float cold, xj, xi, xf, jn, aj, i, f, craw, xo, xc, on, cn;
};

template <bool NORM, bool PEEP, int ACT>
__device__ __forceinline__ void lstm_element(const LstmArgs &a, const CellIdx &ix, int it, const float2 (&sa)[3], const float2 (&sb)[2], LstmEl &r)
{
    const int ch = ix.ch[it], F = a.F;
    const float *yp = a.y + ix.yoff[it] * a.ys + ch;
    r.cold = a.c[ix.eoff[it]];
    float j = yp[0], i = yp[F], f = yp[2 * F], o = yp[3 * F];
    if (PEEP) {
        i += a.wci[ix.e[it]] * r.cold;
        f += a.wcf[ix.e[it]] * r.cold;
    }
    r.xj = r.xi = r.xf = r.xo = r.xc = 0.f;
    if (NORM) {
        r.xj = ln_xhat(j, sa[0]); r.xi = ln_xhat(i, sa[1]); r.xf = ln_xhat(f, sa[2]);
        j = r.xj * a.gamma[ch] + a.beta[ch];
        i = r.xi * a.gamma[F + ch] + a.beta[F + ch];
        f = r.xf * a.gamma[2 * F + ch] + a.beta[2 * F + ch];
    }
    r.jn = j;
    r.aj = cell_act<ACT>(j);
    r.f = cell_sigmoid(f + a.forget_bias);
    r.i = cell_sigmoid(i);
    r.craw = r.cold * r.f + r.i * r.aj;
    if (PEEP) o += a.wco[ix.e[it]] * r.craw;
    r.on = o; r.cn = r.craw;
    if (NORM) {
        r.xo = ln_xhat(o, sb[0]); r.xc = ln_xhat(r.craw, sb[1]);
        r.on = r.xo * a.gamma[3 * F + ch] + a.beta[3 * F + ch];
        r.cn = r.xc * a.gamma[4 * F + ch] + a.beta[4 * F + ch];
    }
}

// do_n = dh' act(c_n) sigmoid'(o_n),  dc_n = dc' + dh' sigmoid(o_n) act'(c_n)
template <int ACT> __device__ __forceinline__ void lstm_output_adjoint(const LstmBwdArgs &a, const CellIdx &ix, int it, const LstmEl &r, float &don, float &dcn)
{
    const float dh = a.dh ? a.dh[ix.yoff[it] * a.dhs + ix.ch[it]] : 0.f;
    const float so = cell_sigmoid(r.on), ac = cell_act<ACT>(r.cn);
    don = dh * ac * sigmoid_grad(so);
    dcn = (a.dcn ? a.dcn[ix.eoff[it]] : 0.f) + dh * so * cell_act_grad<ACT>(r.cn, ac);
}

__device__ __forceinline__ void lstm_load_stats(const LstmArgs &a, float2 (&sa)[3], float2 (&sb)[2])
{
#pragma unroll
    for (int q = 0; q < 3; ++q) sa[q] = a.stats_a[blockIdx.y * 3 + q];
#pragma unroll
    for (int q = 0; q < 2; ++q) sb[q] = a.stats_b[blockIdx.y * 2 + q];
}

// backward A (normalize only): chunk sums of g and g xhat for the layer norms of o and c'; their gamma / beta products
template <bool PEEP, int ACT> __global__ __launch_bounds__(256) void lstm_bwd_a_kernel(LstmBwdArgs a)
{
    __shared__ double red[16];
    CellIdx ix;
    cell_index(a.f.HW, a.f.F, ix);
    float2 sa[3], sb[2];
    lstm_load_stats(a.f, sa, sb);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int it = 0; it < CELL_E; ++it) {
        if (!ix.ok[it]) continue;
        const int ch = ix.ch[it], F = a.f.F;
        LstmEl r;
        lstm_element<true, PEEP, ACT>(a.f, ix, it, sa, sb, r);
        float don, dcn;
        lstm_output_adjoint<ACT>(a, ix, it, r, don, dcn);
        const float go = don * a.f.gamma[3 * F + ch], gc = dcn * a.f.gamma[4 * F + ch];
        acc[0] += go; acc[1] += go * r.xo; acc[2] += gc; acc[3] += gc * r.xc;
        if (a.prod) {
            prod_store(a.prod, ix.yoff[it], 5, F, 3, ch, don, r.xo);
            prod_store(a.prod, ix.yoff[it], 5, F, 4, ch, dcn, r.xc);
        }
    }
    chunk_sums<4>(acc, a.part1, red);
}

// backward B: through the output stage and the state update.  Writes do (final), d c (its part through f), c' before its layer norm,
// and dj, di, df with respect to the layer norms' outputs -- NORM: with their chunk sums and products, for C; otherwise they are
// final and the peepholes' part of d c is added here
template <bool NORM, bool PEEP, int ACT> __global__ __launch_bounds__(256) void lstm_bwd_b_kernel(LstmBwdArgs a)
{
    __shared__ double red[24];
    CellIdx ix;
    cell_index(a.f.HW, a.f.F, ix);
    float2 sa[3], sb[2];
    float m1[4] = {0.f, 0.f, 0.f, 0.f};
    if (NORM) {
        lstm_load_stats(a.f, sa, sb);
#pragma unroll
        for (int q = 0; q < 4; ++q) m1[q] = a.sums1[blockIdx.y * 4 + q];
    }
    float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int it = 0; it < CELL_E; ++it) {
        if (!ix.ok[it]) continue;
        const int ch = ix.ch[it], F = a.f.F;
        LstmEl r;
        lstm_element<NORM, PEEP, ACT>(a.f, ix, it, sa, sb, r);
        float d_o, d_c;
        lstm_output_adjoint<ACT>(a, ix, it, r, d_o, d_c);
        if (NORM) {
            d_o = ln_apply_adjoint(d_o, a.f.gamma[3 * F + ch], r.xo, sb[0].y, m1[0], m1[1]);
            d_c = ln_apply_adjoint(d_c, a.f.gamma[4 * F + ch], r.xc, sb[1].y, m1[2], m1[3]);
        }
        if (PEEP) d_c += a.f.wco[ix.e[it]] * d_o;
        const float dj = d_c * r.i * cell_act_grad<ACT>(r.jn, r.aj);
        const float di = d_c * r.aj * sigmoid_grad(r.i);
        const float df = d_c * r.cold * sigmoid_grad(r.f);
        float dcold = d_c * r.f;
        float *dyp = a.dy + ix.yoff[it] * a.dys + ch;
        dyp[0] = dj; dyp[F] = di; dyp[2 * F] = df; dyp[3 * F] = d_o;
        if (ch == 0) zero_pads(dyp, 4 * F, a.dys);
        if (a.c_raw) a.c_raw[ix.eoff[it]] = r.craw;
        if (NORM) {
            const float gj = dj * a.f.gamma[ch], gi = di * a.f.gamma[F + ch], gf = df * a.f.gamma[2 * F + ch];
            acc[0] += gj; acc[1] += gj * r.xj; acc[2] += gi; acc[3] += gi * r.xi; acc[4] += gf; acc[5] += gf * r.xf;
            if (a.prod) {
                prod_store(a.prod, ix.yoff[it], 5, F, 0, ch, dj, r.xj);
                prod_store(a.prod, ix.yoff[it], 5, F, 1, ch, di, r.xi);
                prod_store(a.prod, ix.yoff[it], 5, F, 2, ch, df, r.xf);
            }
        } else if (PEEP) {
            dcold += a.f.wci[ix.e[it]] * di + a.f.wcf[ix.e[it]] * df;
        }
        a.dc[ix.eoff[it]] = dcold;
    }
    if (NORM) chunk_sums<6>(acc, a.part2, red);
}

// backward C (normalize only): dj, di, df through their layer norms, in place; the peepholes' part of d c
template <bool PEEP> __global__ __launch_bounds__(256) void lstm_bwd_c_kernel(LstmBwdArgs a)
{
    CellIdx ix;
    cell_index(a.f.HW, a.f.F, ix);
    float2 sa[3];
    float m2[6];
#pragma unroll
    for (int q = 0; q < 3; ++q) sa[q] = a.f.stats_a[blockIdx.y * 3 + q];
#pragma unroll
    for (int q = 0; q < 6; ++q) m2[q] = a.sums2[blockIdx.y * 6 + q];
#pragma unroll
    for (int it = 0; it < CELL_E; ++it) {
        if (!ix.ok[it]) continue;
        const int ch = ix.ch[it], F = a.f.F;
        const float *yp = a.f.y + ix.yoff[it] * a.f.ys + ch;
        float v[3] = {yp[0], yp[F], yp[2 * F]};
        if (PEEP) {
            const float cold = a.f.c[ix.eoff[it]];
            v[1] += a.f.wci[ix.e[it]] * cold;
            v[2] += a.f.wcf[ix.e[it]] * cold;
        }
        float *dyp = a.dy + ix.yoff[it] * a.dys + ch;
        float d[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            d[q] = ln_apply_adjoint(dyp[q * F], a.f.gamma[q * F + ch], ln_xhat(v[q], sa[q]), sa[q].y, m2[2 * q], m2[2 * q + 1]);
            dyp[q * F] = d[q];
        }
        if (PEEP) a.dc[ix.eoff[it]] += a.f.wci[ix.e[it]] * d[1] + a.f.wcf[ix.e[it]] * d[2];
    }
}

// peephole gradients: one thread per element e of [H, W, F], the samples in order, summed in double.
// dW_ci[e] (+)= sum_b di[b,e] c[b,e], dW_cf with df, dW_co[e] (+)= sum_b do[b,e] c_raw[b,e]
__global__ __launch_bounds__(256) void lstm_peephole_grad_kernel(const float *__restrict__ dy, int dys, const float *__restrict__ c,
                                                                 const float *__restrict__ c_raw, int B, int HW, int F,
                                                                 float *__restrict__ dwci, float *__restrict__ dwcf, float *__restrict__ dwco,
                                                                 int accumulate)
{
    const int N = HW * F, e = blockIdx.x * 256 + (int)threadIdx.x;
    if (e >= N) return;
    const int px = e / F, ch = e - px * F;
    double si = 0.0, sf = 0.0, so = 0.0;              // (the products in float, as everywhere; their sums in double, rounded once)
    for (int b = 0; b < B; ++b) {
        const float *dyp = dy + ((unsigned)b * HW + px) * dys + ch;
        const float cold = c[(unsigned)b * N + e];
        si += (double)(dyp[F] * cold);
        sf += (double)(dyp[2 * F] * cold);
        so += (double)(dyp[3 * F] * c_raw[(unsigned)b * N + e]);
    }
    if (accumulate) { si += (double)dwci[e]; sf += (double)dwcf[e]; so += (double)dwco[e]; }
    dwci[e] = (float)si; dwcf[e] = (float)sf; dwco[e] = (float)so;
}

struct GruBwdArgs {
    const float *y; int ys;                       // gates: r, u at channels 0, F; update: the candidate at channel 0
    const float *h; int hs;                       // the old state as a slice
    const float *u;                               // update: [B, N]
    const float *gamma, *beta;
    const float2 *stats;                          // the forward's: gates [B][2], update [B][1]
    int HW, F;
    const float *dhn; int dhns;                   // update: d h' as a slice
    const float *du_in;                           // gates: d u [B, N]
    const float *drh; int drhs;                   // gates: d (r h) as a slice
    float *dy; int dys;                           // gates: [dr, du]; update: d y2
    float *du;                                    // update: [B, N]
    float *dh; int dhs;                           // update: d h = d h' u (written); gates: d h += d(r h) r
    float *prod;                                  // [B*HW, 2 Q F] or NULL
    double *part;
    const float *sums;                            // [B][2 Q]
};

// update, first pass: du = dh' (h - act(y2_n)), dh = dh' u, dy2_n = dh' (1 - u) act'(y2_n) (final without NORM)
template <bool NORM, int ACT> __global__ __launch_bounds__(256) void gru_update_bwd_kernel(GruBwdArgs a)
{
    __shared__ double red[8];
    CellIdx ix;
    cell_index(a.HW, a.F, ix);
    float2 sy = make_float2(0.f, 0.f);
    if (NORM) sy = a.stats[blockIdx.y];
    float acc[2] = {0.f, 0.f};
#pragma unroll
    for (int it = 0; it < CELL_E; ++it) {
        if (!ix.ok[it]) continue;
        const int ch = ix.ch[it];
        float y2 = a.y[ix.yoff[it] * a.ys + ch], xh = 0.f;
        if (NORM) {
            xh = ln_xhat(y2, sy);
            y2 = xh * a.gamma[ch] + a.beta[ch];
        }
        const float u = a.u[ix.eoff[it]], h = a.h[ix.yoff[it] * a.hs + ch], dhn = a.dhn[ix.yoff[it] * a.dhns + ch];
        const float ay = cell_act<ACT>(y2);
        const float dy2 = dhn * (1.0f - u) * cell_act_grad<ACT>(y2, ay);
        a.du[ix.eoff[it]] = dhn * (h - ay);
        a.dh[ix.yoff[it] * a.dhs + ch] = dhn * u;
        float *dyp = a.dy + ix.yoff[it] * a.dys + ch;
        dyp[0] = dy2;
        if (ch == 0) zero_pads(dyp, a.F, a.dys);
        if (NORM) {
            const float g = dy2 * a.gamma[ch];
            acc[0] += g; acc[1] += g * xh;
            if (a.prod) prod_store(a.prod, ix.yoff[it], 1, a.F, 0, ch, dy2, xh);
        }
    }
    if (NORM) chunk_sums<2>(acc, a.part, red);
}

// gates, first pass: dr_n = d(r h) h sigmoid'(r), du_n = du sigmoid'(u) (final without NORM), dh += d(r h) r
template <bool NORM> __global__ __launch_bounds__(256) void gru_gates_bwd_kernel(GruBwdArgs a)
{
    __shared__ double red[16];
    CellIdx ix;
    cell_index(a.HW, a.F, ix);
    float2 sr = make_float2(0.f, 0.f), su = sr;
    if (NORM) { sr = a.stats[blockIdx.y * 2]; su = a.stats[blockIdx.y * 2 + 1]; }
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int it = 0; it < CELL_E; ++it) {
        if (!ix.ok[it]) continue;
        const int ch = ix.ch[it], F = a.F;
        const float *yp = a.y + ix.yoff[it] * a.ys + ch;
        float r = yp[0], u = yp[F], xr = 0.f, xu = 0.f;
        if (NORM) {
            xr = ln_xhat(r, sr); xu = ln_xhat(u, su);
            r = xr * a.gamma[ch] + a.beta[ch];
            u = xu * a.gamma[F + ch] + a.beta[F + ch];
        }
        r = cell_sigmoid(r);
        u = cell_sigmoid(u);
        const float h = a.h[ix.yoff[it] * a.hs + ch], drh = a.drh[ix.yoff[it] * a.drhs + ch];
        const float dr = drh * h * sigmoid_grad(r), du = a.du_in[ix.eoff[it]] * sigmoid_grad(u);
        a.dh[ix.yoff[it] * a.dhs + ch] += drh * r;
        float *dyp = a.dy + ix.yoff[it] * a.dys + ch;
        dyp[0] = dr; dyp[F] = du;
        if (ch == 0) zero_pads(dyp, 2 * F, a.dys);
        if (NORM) {
            const float gr = dr * a.gamma[ch], gu = du * a.gamma[F + ch];
            acc[0] += gr; acc[1] += gr * xr; acc[2] += gu; acc[3] += gu * xu;
            if (a.prod) {
                prod_store(a.prod, ix.yoff[it], 2, F, 0, ch, dr, xr);
                prod_store(a.prod, ix.yoff[it], 2, F, 1, ch, du, xu);
            }
        }
    }
    if (NORM) chunk_sums<4>(acc, a.part, red);
}

// second pass of both GRU stages: the Q gates of dy through their layer norms, in place
template <int Q> __global__ __launch_bounds__(256) void gru_ln_bwd_kernel(GruBwdArgs a)
{
    CellIdx ix;
    cell_index(a.HW, a.F, ix);
    float2 st[Q];
    float m[2 * Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) st[q] = a.stats[blockIdx.y * Q + q];
#pragma unroll
    for (int q = 0; q < 2 * Q; ++q) m[q] = a.sums[blockIdx.y * 2 * Q + q];
#pragma unroll
    for (int it = 0; it < CELL_E; ++it) {
        if (!ix.ok[it]) continue;
        const int ch = ix.ch[it];
        const float *yp = a.y + ix.yoff[it] * a.ys + ch;
        float *dyp = a.dy + ix.yoff[it] * a.dys + ch;
#pragma unroll
        for (int q = 0; q < Q; ++q)
            dyp[q * a.F] = ln_apply_adjoint(dyp[q * a.F], a.gamma[q * a.F + ch], ln_xhat(yp[q * a.F], st[q]), st[q].y, m[2 * q], m[2 * q + 1]);
    }
}

// row chunks of the gamma / beta column sums: 64 rows or more each, at most 128 chunks
inline int cell_colsum_chunks(long long rows) { return (int)(rows < 64 * 128 ? (rows + 63) / 64 : 128); }

// the backward workspace of one call, carved the same way by the size functions and the launchers.  q1, q2: sums of the first and
// second reduction; nln: layer norms with parameter gradients (0: no product table); craw: the LSTM's c' before its layer norm
struct CellBwdWs { size_t part1, part2, sums1, sums2, prod, c_raw, colsum, total; };

CellBwdWs cell_bwd_ws(int B, int HW, int F, int q1, int q2, int nln, bool craw)
{
    CellBwdWs w{};
    const size_t nch = (size_t)cell_chunks(HW * F), rows = (size_t)B * HW;
    size_t off = 0;
    w.part1 = off; off += up256((size_t)B * q1 * nch * sizeof(double));
    w.part2 = off; off += up256((size_t)B * q2 * nch * sizeof(double));
    w.sums1 = off; off += up256((size_t)B * q1 * sizeof(float));
    w.sums2 = off; off += up256((size_t)B * q2 * sizeof(float));
    w.prod = off; off += up256(rows * 2 * nln * F * sizeof(float));
    w.c_raw = off; off += craw ? up256(rows * F * sizeof(float)) : 0;
    w.colsum = off; off += nln ? up256((size_t)cell_colsum_chunks((long long)rows) * 2 * nln * F * sizeof(double)) : 0;
    w.total = off;
    return w;
}

// dgamma [Q][F] and dbeta [Q][F] from the product table: grid (ceil(2QF / 64), chunks); a workgroup sums the rows of its chunk for 64
// columns in double (consecutive lanes on consecutive columns, four rows at a time) into part[chunk][column]; the final kernel adds
// the chunks in order
__global__ __launch_bounds__(256) void cell_colsum_kernel(const float *__restrict__ prod, long long rows, int rows_per_chunk, int C,
                                                          double *__restrict__ part)
{
    __shared__ double red[4][64];
    const int cl = threadIdx.x & 63, rp = threadIdx.x >> 6, c = blockIdx.x * 64 + cl;
    const long long r0 = (long long)blockIdx.y * rows_per_chunk, r1 = r0 + rows_per_chunk < rows ? r0 + rows_per_chunk : rows;
    double acc = 0.0;
    if (c < C)
        for (long long r = r0 + rp; r < r1; r += 4) acc += (double)prod[(size_t)r * C + c];
    red[rp][cl] = acc;
    __syncthreads();
    if (rp == 0 && c < C) part[(size_t)blockIdx.y * C + c] = (red[0][cl] + red[1][cl]) + (red[2][cl] + red[3][cl]);
}

__global__ __launch_bounds__(256) void cell_colsum_final_kernel(const double *__restrict__ part, int chunks, int C, int half, float *__restrict__ dgamma,
                                                                float *__restrict__ dbeta, int accumulate)
{
    const int c = blockIdx.x * 256 + (int)threadIdx.x;
    if (c >= C) return;
    double s = 0.0;
    for (int k = 0; k < chunks; ++k) s += part[(size_t)k * C + c];
    float *out = c < half ? dgamma + c : dbeta + (c - half);
    *out = (float)(accumulate ? s + (double)*out : s);
}

hipError_t cell_param_sums(const float *prod, int B, int HW, int F, int Q, float *dgamma, float *dbeta, int accumulate, double *scratch,
                           hipStream_t stream)
{
    const long long rows = (long long)B * HW;
    const int C = 2 * Q * F, chunks = cell_colsum_chunks(rows), rpc = (int)((rows + chunks - 1) / chunks);
    cell_colsum_kernel<<<dim3((unsigned)((C + 63) / 64), (unsigned)chunks), dim3(256), 0, stream>>>(prod, rows, rpc, C, scratch);
    cell_colsum_final_kernel<<<dim3((unsigned)((C + 255) / 256)), dim3(256), 0, stream>>>(scratch, chunks, C, Q * F, dgamma, dbeta, accumulate);
    return hipGetLastError();
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

// ---------------------------------------------------------------------------------------------------------------- backward
size_t convlstm_stats_offset(int B, int HW, int F, int which)
{
    const CellWs w = cell_ws(B, HW * F, 3, 2, true);
    return which == 0 ? w.stats_a : w.stats_b;
}

size_t convgru_stats_offset(int B, int HW, int F) { return cell_ws(B, HW * F, 2, 0, false).stats_a; }

size_t convlstm_backward_workspace_bytes(int B, int HW, int F, bool normalize, bool peephole)
{
    return cell_bwd_ws(B, HW, F, normalize ? 4 : 0, normalize ? 6 : 0, normalize ? 5 : 0, peephole).total;
}

size_t convgru_backward_workspace_bytes(int B, int HW, int F, bool normalize)
{
    if (!normalize) return 0;
    const size_t gates = cell_bwd_ws(B, HW, F, 4, 0, 2, false).total, update = cell_bwd_ws(B, HW, F, 2, 0, 1, false).total;
    return gates > update ? gates : update;                    // each call carves its own: one workspace serves both
}

hipError_t launch_convlstm_gates_backward(const float *y, int ys, const float *c, const float *wci, const float *wcf, const float *wco,
                                          const float *gamma, const float *beta, const float *stats_jif, const float *stats_oc, const float *dh,
                                          int dhs, const float *dc_new, int B, int HW, int F, float forget_bias, int act, bool normalize,
                                          bool peephole, float *dy, int dys, float *dc, float *dwci, float *dwcf, float *dwco, float *dgamma,
                                          float *dbeta, int accumulate, void *workspace, hipStream_t stream)
{
    const int N = HW * F;
    const CellBwdWs w = cell_bwd_ws(B, HW, F, normalize ? 4 : 0, normalize ? 6 : 0, normalize ? 5 : 0, peephole);
    char *ws = reinterpret_cast<char *>(workspace);
    LstmBwdArgs a{};
    a.f.y = y; a.f.ys = ys; a.f.c = c; a.f.wci = wci; a.f.wcf = wcf; a.f.wco = wco; a.f.gamma = gamma; a.f.beta = beta; a.f.HW = HW; a.f.F = F;
    a.f.forget_bias = forget_bias;
    a.f.stats_a = reinterpret_cast<const float2 *>(stats_jif); a.f.stats_b = reinterpret_cast<const float2 *>(stats_oc);
    a.dh = dh; a.dhs = dhs; a.dcn = dc_new; a.dy = dy; a.dys = dys; a.dc = dc;
    const bool want_peep = peephole && dwci;
    a.c_raw = want_peep ? reinterpret_cast<float *>(ws + w.c_raw) : nullptr;
    const dim3 grid = cell_grid(B, N), blk(256);
    if (normalize) {
        a.prod = dgamma ? reinterpret_cast<float *>(ws + w.prod) : nullptr;
        a.part1 = reinterpret_cast<double *>(ws + w.part1);
        a.part2 = reinterpret_cast<double *>(ws + w.part2);
        a.sums1 = reinterpret_cast<const float *>(ws + w.sums1);
        a.sums2 = reinterpret_cast<const float *>(ws + w.sums2);
#define CALL(A)                                                                     \
    if (peephole) lstm_bwd_a_kernel<true, A><<<grid, blk, 0, stream>>>(a);          \
    else lstm_bwd_a_kernel<false, A><<<grid, blk, 0, stream>>>(a)
        CELL_FOR_ACT(act, CALL)
#undef CALL
        cell_sums_kernel<<<dim3(4, (unsigned)B), dim3(64), 0, stream>>>(a.part1, (int)grid.x, N, reinterpret_cast<float *>(ws + w.sums1));
#define CALL(A)                                                                     \
    if (peephole) lstm_bwd_b_kernel<true, true, A><<<grid, blk, 0, stream>>>(a);    \
    else lstm_bwd_b_kernel<true, false, A><<<grid, blk, 0, stream>>>(a)
        CELL_FOR_ACT(act, CALL)
#undef CALL
        cell_sums_kernel<<<dim3(6, (unsigned)B), dim3(64), 0, stream>>>(a.part2, (int)grid.x, N, reinterpret_cast<float *>(ws + w.sums2));
        if (peephole) lstm_bwd_c_kernel<true><<<grid, blk, 0, stream>>>(a);
        else lstm_bwd_c_kernel<false><<<grid, blk, 0, stream>>>(a);
    } else {
#define CALL(A)                                                                     \
    if (peephole) lstm_bwd_b_kernel<false, true, A><<<grid, blk, 0, stream>>>(a);   \
    else lstm_bwd_b_kernel<false, false, A><<<grid, blk, 0, stream>>>(a)
        CELL_FOR_ACT(act, CALL)
#undef CALL
    }
    if (want_peep)
        lstm_peephole_grad_kernel<<<dim3((unsigned)((N + 255) / 256)), blk, 0, stream>>>(dy, dys, c, a.c_raw, B, HW, F, dwci, dwcf, dwco, accumulate);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && normalize && dgamma)
        e = cell_param_sums(a.prod, B, HW, F, 5, dgamma, dbeta, accumulate, reinterpret_cast<double *>(ws + w.colsum), stream);
    return e;
}

hipError_t launch_convgru_update_backward(const float *y2, int ys, const float *h, int hs, const float *u, const float *gamma, const float *beta,
                                          const float *stats, const float *dh_new, int dhns, int B, int HW, int F, int act, bool normalize,
                                          float *dy2, int dys, float *du, float *dh, int dhs, float *dgamma, float *dbeta, int accumulate,
                                          void *workspace, hipStream_t stream)
{
    const int N = HW * F;
    GruBwdArgs a{};
    a.y = y2; a.ys = ys; a.h = h; a.hs = hs; a.u = u; a.gamma = gamma; a.beta = beta; a.stats = reinterpret_cast<const float2 *>(stats);
    a.HW = HW; a.F = F; a.dhn = dh_new; a.dhns = dhns; a.dy = dy2; a.dys = dys; a.du = du; a.dh = dh; a.dhs = dhs;
    const dim3 grid = cell_grid(B, N), blk(256);
    if (!normalize) {
#define CALL(A) gru_update_bwd_kernel<false, A><<<grid, blk, 0, stream>>>(a)
        CELL_FOR_ACT(act, CALL)
#undef CALL
        return hipGetLastError();
    }
    const CellBwdWs w = cell_bwd_ws(B, HW, F, 2, 0, 1, false);
    char *ws = reinterpret_cast<char *>(workspace);
    a.prod = dgamma ? reinterpret_cast<float *>(ws + w.prod) : nullptr;
    a.part = reinterpret_cast<double *>(ws + w.part1);
    a.sums = reinterpret_cast<const float *>(ws + w.sums1);
#define CALL(A) gru_update_bwd_kernel<true, A><<<grid, blk, 0, stream>>>(a)
    CELL_FOR_ACT(act, CALL)
#undef CALL
    cell_sums_kernel<<<dim3(2, (unsigned)B), dim3(64), 0, stream>>>(a.part, (int)grid.x, N, reinterpret_cast<float *>(ws + w.sums1));
    gru_ln_bwd_kernel<1><<<grid, blk, 0, stream>>>(a);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && dgamma) e = cell_param_sums(a.prod, B, HW, F, 1, dgamma, dbeta, accumulate, reinterpret_cast<double *>(ws + w.colsum), stream);
    return e;
}

hipError_t launch_convgru_gates_backward(const float *y, int ys, const float *h, int hs, const float *gamma, const float *beta, const float *stats,
                                         const float *du, const float *drh, int drhs, int B, int HW, int F, bool normalize, float *dy, int dys,
                                         float *dh, int dhs, float *dgamma, float *dbeta, int accumulate, void *workspace, hipStream_t stream)
{
    const int N = HW * F;
    GruBwdArgs a{};
    a.y = y; a.ys = ys; a.h = h; a.hs = hs; a.gamma = gamma; a.beta = beta; a.stats = reinterpret_cast<const float2 *>(stats);
    a.HW = HW; a.F = F; a.du_in = du; a.drh = drh; a.drhs = drhs; a.dy = dy; a.dys = dys; a.dh = dh; a.dhs = dhs;
    const dim3 grid = cell_grid(B, N), blk(256);
    if (!normalize) {
        gru_gates_bwd_kernel<false><<<grid, blk, 0, stream>>>(a);
        return hipGetLastError();
    }
    const CellBwdWs w = cell_bwd_ws(B, HW, F, 4, 0, 2, false);
    char *ws = reinterpret_cast<char *>(workspace);
    a.prod = dgamma ? reinterpret_cast<float *>(ws + w.prod) : nullptr;
    a.part = reinterpret_cast<double *>(ws + w.part1);
    a.sums = reinterpret_cast<const float *>(ws + w.sums1);
    gru_gates_bwd_kernel<true><<<grid, blk, 0, stream>>>(a);
    cell_sums_kernel<<<dim3(4, (unsigned)B), dim3(64), 0, stream>>>(a.part, (int)grid.x, N, reinterpret_cast<float *>(ws + w.sums1));
    gru_ln_bwd_kernel<2><<<grid, blk, 0, stream>>>(a);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && dgamma) e = cell_param_sums(a.prod, B, HW, F, 2, dgamma, dbeta, accumulate, reinterpret_cast<double *>(ws + w.colsum), stream);
    return e;
}

}  // namespace vstab
