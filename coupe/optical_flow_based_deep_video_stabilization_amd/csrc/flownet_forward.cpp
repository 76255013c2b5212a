// The FlowNetS pyramid on the GPU: weight packing / upload, the forward schedule (model.py:786-893) over the plan of flownet_plan.cpp,
// its per-launch profiling, and the entry points that run the evaluator's tail in the forward's last launch.
#include <cmath>
#include <cstdlib>
#include <memory>

#include "flownet_plan.h"

using namespace vstab;

static const char *UP_NAME[4] = {"upsample6_5", "upsample5_4", "upsample4_3", "upsample3_2"};

// ------------------------------------------------------------------------- weights
extern "C" int vstab_load_weights(vstab_ctx *ctx, const vstab_tensor *t, int count)
{
    if (!ctx) return fail(nullptr, VSTAB_E_STATE, "vstab_load_weights: ctx is NULL");
    if (!t || count <= 0) return fail(ctx, VSTAB_E_WEIGHTS, "vstab_load_weights: no tensors");
    const vstab_tensor *w1 = find(t, count, "1/W_conv2d");
    if (!w1 || w1->ndim != 4) return fail(ctx, VSTAB_E_WEIGHTS, "missing variable 1/W_conv2d");
    const int cin = w1->shape[2];
    if (cin < 1 || cin > 4096) return fail(ctx, VSTAB_E_WEIGHTS, "1/W_conv2d: bad Cin %d", cin);

    std::vector<float> host;
    auto reserve = [&](size_t n) { size_t o = (host.size() + 63) / 64 * 64; host.resize(o + n, 0.f); return o; };
    std::vector<double> scale;
    auto need = [&](const std::string &name, std::initializer_list<int> s) -> const vstab_tensor * {
        const vstab_tensor *x = find(t, count, name);
        return shape_is(x, s) ? x : nullptr;
    };
#define NEED(var, name, ...)                                                                   \
    const vstab_tensor *var = need(name, {__VA_ARGS__});                                        \
    if (!var) return fail(ctx, VSTAB_E_WEIGHTS, "missing or mis-shaped variable %s", std::string(name).c_str());

    // encoder
    for (int i = 0; i < 10; ++i) {
        const Layer &e = NET[i];
        const int ci = i == 0 ? cin : e.cin;
        const int cs_in = i == 0 ? cin : in_buf(e).cs;
        const std::string n = e.name + 4;                 // variables "1/...", "3_1/..."
        NEED(W, n + "/W_conv2d", e.k, e.k, ci, e.cout)
        NEED(b, n + "/b_conv2d", e.cout)
        NEED(beta, n + "/beta", e.cout)
        NEED(mean, n + "/moving_mean", e.cout)
        NEED(var, n + "/moving_variance", e.cout)
        const int npad = padded_cols(e.cout);
        const KLayout L = conv_layout(e.k, e.k, ci, cs_in);
        scale.assign(npad, 1.0);
        ctx->enc_b[i] = reserve(npad);
        fold_bn(b->data, beta->data, mean->data, var->data, e.cout, npad, scale.data(), host.data() + ctx->enc_b[i]);
        ctx->enc_w[i] = reserve((size_t)L.ktiles() * npad * 32);
        pack_conv(W->data, scale.data(), e.k, e.k, ci, cs_in, e.cout, npad, L, host.data() + ctx->enc_w[i]);
        if (e.k == 3 && e.s == 1 && (ci & 31) == 0 && (e.cout & 127) == 0) {      // Winograd-domain operands (16 positions)
            ctx->wino_w[i] = reserve((size_t)16 * (ci / 32) * e.cout * 32);
            pack_winograd(W->data, scale.data(), ci, e.cout, e.cout, host.data() + ctx->wino_w[i]);
        }
        if (i == 0) {
            const int lead = rowwin_lead(-e.p, cin), segp = rowwin_segp(-e.p, e.k, cin);
            ctx->enc0_rw = reserve((size_t)e.k * (segp / 32) * npad * 32);
            pack_conv_rowwin(W->data, scale.data(), e.k, e.k, cin, e.cout, npad, lead, segp, host.data() + ctx->enc0_rw);
            ctx->enc0_b3 = 0;
            if (npad == 64) {                    // the same K order as three bf16 planes (two bf16 per float of the blob)
                ctx->enc0_b3 = reserve((size_t)e.k * (segp / 16) * 3 * 64 * 16 / 2);
                pack_conv1_bf16x3(W->data, scale.data(), e.k, e.k, cin, e.cout, lead, segp, reinterpret_cast<uint16_t *>(host.data() + ctx->enc0_b3));
            }
        }
    }
    // decoder
    for (int l = 0; l < 4; ++l) {
        const Layer &d = dec_layer(l);
        const std::string n = d.name;
        const int co = d.cout, ci = d.cin, cs = in_buf(d).cs;
        NEED(W, n + "/W_deconv2d", 4, 4, co, ci)
        NEED(b, n + "/b_deconv2d", co)
        NEED(beta, n + "_bn/beta", co)
        NEED(mean, n + "_bn/moving_mean", co)
        NEED(var, n + "_bn/moving_variance", co)
        const int npad = padded_cols(co);
        scale.assign(npad, 1.0);
        ctx->dec_b[l] = reserve(npad);
        fold_bn(b->data, beta->data, mean->data, var->data, co, npad, scale.data(), host.data() + ctx->dec_b[l]);
        ctx->dec_w[l] = reserve(4 * (size_t)klayout_deconv(cs).ktiles() * npad * 32);
        pack_deconv(W->data, scale.data(), ci, cs, co, npad, host.data() + ctx->dec_w[l]);
        ctx->wdec_w[l] = 0;
        if (l <= 2) {                 // Winograd F(2x2,2x2)-domain operands (9 positions x 4 phases) of the levels wdec_applies() can choose
            ctx->wdec_w[l] = reserve(9 * (size_t)klayout_run(1, 1, cs).ktiles() * 4 * co * 32);
            pack_wdec(W->data, scale.data(), ci, cs, co, host.data() + ctx->wdec_w[l]);
        }

        const std::string u = UP_NAME[l];
        NEED(uw, u + "/W_deconv2d", 4, 4, 2, 2)
        NEED(ub, u + "/b_deconv2d", 2)
        std::memcpy(ctx->up[l].w, uw->data, sizeof(float) * 64);
        ctx->up[l].b[0] = ub->data[0]; ctx->up[l].b[1] = ub->data[1];
    }
    // predict heads
    for (int l = 0; l < 4; ++l) {
        const Layer &h = head_layer(l);
        const std::string n = h.name;
        NEED(W, n + "/W_conv2d", 3, 3, h.cin, 2)
        NEED(b, n + "/b_conv2d", 2)
        ctx->pred_w[l] = reserve((size_t)klayout_run(1, 1, in_buf(h).cs).ktiles() * 32 * 32);
        pack_predict2_table(W->data, h.cin, in_buf(h).cs, 32, host.data() + ctx->pred_w[l]);
        ctx->pred_b[l] = reserve(4);
        host[ctx->pred_b[l]] = b->data[0]; host[ctx->pred_b[l] + 1] = b->data[1];
    }
    {
        NEED(W, "predict2/W_conv2d", 3, 3, NET[14].cin, 2)
        NEED(b, "predict2/b_conv2d", 2)
        ctx->tab_b = reserve(32);
        ctx->tab_wp = reserve((size_t)200 * 32);
        pack_predict2_panel(W->data, NET[14].cin, 200, host.data() + ctx->tab_wp);
        ctx->zero_b = reserve(2048);             // zero bias for the Winograd-domain GEMMs (bias is added by the inverse transform)
        ctx->pred2_b = reserve(4);
        host[ctx->pred2_b] = b->data[0]; host[ctx->pred2_b + 1] = b->data[1];
    }
#undef NEED

    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (ctx->dev_weights) { (void)hipFree(ctx->dev_weights); ctx->dev_weights = nullptr; }
    ctx->loaded = false;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&ctx->dev_weights), host.size() * sizeof(float));
    if (e != hipSuccess) return fail(ctx, VSTAB_E_NOMEM, "hipMalloc(%zu bytes of packed weights): %s", host.size() * 4, hipGetErrorString(e));
    HIP_TRY(ctx, hipMemcpy(ctx->dev_weights, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
    ctx->dev_weight_floats = host.size();
    ctx->cin = cin;
    ctx->loaded = true;
    return VSTAB_OK;
}

// ------------------------------------------------------------------------- forward
// evaluate_originalSize's tail riding in the forward: when given, the last launch of a chunk computes predict_flow2, the flow glue and
// tf_warp of the chunk's frames together (launch_pf2_glue_warp); `fused` reports whether every chunk could (else the caller warps)
struct FusedTail { const float *frame; float *outflow; float *warped; int oh, ow; bool fused; const uint8_t *frame8; uint8_t *out8; };      // fp32 frames, or the clip driver's 8-bit ones (frame8 / out8)
static int forward_chunk(vstab_ctx *ctx, const float *feats, int B, int H, int W, int Cin, float *pf6, float *pf5,
                         float *pf4, float *pf3, float *pf2, void *workspace, size_t workspace_bytes, void *stream_, FusedTail *tail);
static const char *conv_kernel_name(ConvTile t, bool vec4);
static const char *dual_kernel_name(ConvTile t);
static int forward_impl(vstab_ctx *ctx, const float *feats, int B, int H, int W, int Cin, float *pf6, float *pf5, float *pf4, float *pf3,
                        float *pf2, void *workspace, size_t workspace_bytes, void *stream_, FusedTail *tail);

extern "C" int vstab_flownets_forward(vstab_ctx *ctx, const float *feats, int B, int H, int W, int Cin, float *pf6,
                                      float *pf5, float *pf4, float *pf3, float *pf2, void *workspace,
                                      size_t workspace_bytes, void *stream_)
{
    return forward_impl(ctx, feats, B, H, W, Cin, pf6, pf5, pf4, pf3, pf2, workspace, workspace_bytes, stream_, nullptr);
}

static int forward_impl(vstab_ctx *ctx, const float *feats, int B, int H, int W, int Cin, float *pf6, float *pf5, float *pf4, float *pf3,
                        float *pf2, void *workspace, size_t workspace_bytes, void *stream_, FusedTail *tail)
{
    if (!ctx) return fail(nullptr, VSTAB_E_STATE, "forward: ctx is NULL");
    if (!ctx->loaded) return fail(ctx, VSTAB_E_STATE, "forward: vstab_load_weights has not been called");
    if (Cin != ctx->cin) return fail(ctx, VSTAB_E_SHAPE, "forward: feats has %d channels, weights expect %d", Cin, ctx->cin);
    if (!feats || !pf6 || !pf5 || !pf4 || !pf3 || !pf2 || !workspace) return fail(ctx, VSTAB_E_STATE, "forward: NULL buffer");
    int eh[10], ew[10];
    if (B < 1 || !level_sizes(H, W, eh, ew)) return fail(ctx, VSTAB_E_SHAPE, "forward: unsupported problem %dx%dx%dx%d", B, H, W, Cin);
    const PlanPin pin = pin_of(ctx);
    if (pin.batch > 0 && B > pin.batch) return fail(ctx, VSTAB_E_SHAPE, "forward: batch %d exceeds the pinned plan batch %d (vstab_set_plan_batch)", B, pin.batch);
    // samples are independent: process the batch in (equalised) chunks that keep every tensor below
    // 2 GiB; equal chunks share one launch plan, so their results are bit-identical -- and so are ragged ones under a pinned plan batch
    const int chunk = chunk_size(pin, B, H, W, Cin);
    if (chunk < 1) return fail(ctx, VSTAB_E_SHAPE, "forward: one %dx%dx%d sample exceeds the 2 GiB tensor limit", H, W, Cin);
    // a batch processed in several chunks hands every chunk its slice of the frames: the slices keep the fused launch's 16-byte alignment
    // only when a frame is a whole number of 16-byte units (else: the two launches after the last chunk, as before)
    bool all_fused = tail != nullptr && (chunk >= B || ((size_t)tail->oh * tail->ow * 4) % 16 == 0);      // (8-bit frames: 4-byte units; the same test covers them)
    for (int b0 = 0; b0 < B; b0 += chunk) {
        const int bc = std::min(chunk, B - b0);
        FusedTail t{};
        if (tail && all_fused) {
            const size_t px = (size_t)b0 * tail->oh * tail->ow;
            t = FusedTail{tail->frame ? tail->frame + px * 3 : nullptr, tail->outflow ? tail->outflow + px * 2 : nullptr,
                          tail->warped ? tail->warped + px * 3 : nullptr, tail->oh, tail->ow, false,
                          tail->frame8 ? tail->frame8 + px * 3 : nullptr, tail->out8 ? tail->out8 + px * 3 : nullptr};
        }
        const int rc = forward_chunk(ctx, feats + (size_t)b0 * H * W * Cin, bc, H, W, Cin,
                                     pf6 + (size_t)b0 * eh[9] * ew[9] * 2, pf5 + (size_t)b0 * eh[7] * ew[7] * 2,
                                     pf4 + (size_t)b0 * eh[5] * ew[5] * 2, pf3 + (size_t)b0 * eh[3] * ew[3] * 2,
                                     pf2 + (size_t)b0 * (H - 2) * (W - 2) * 2, workspace, workspace_bytes, stream_, (tail && all_fused) ? &t : nullptr);
        if (rc != VSTAB_OK) return rc;
        // the first chunk decides (the geometry is the same for every chunk; a later chunk's frame slice could only differ in alignment,
        // and a whole number of frames keeps a 16-byte aligned base 16-byte aligned when oh*ow*12 is a multiple of 16 -- checked per chunk)
        if (tail && all_fused && !t.fused) {
            if (b0 != 0) return fail(ctx, VSTAB_E_ALIGN, "stabilise: chunk %d of the batch misses the fused tail's alignment", b0 / chunk);
            all_fused = false;
        }
    }
    if (tail) tail->fused = all_fused;
    return VSTAB_OK;
}

// The first layer on a row-window kernel, when its alignment conditions hold (*launched): six bf16 piece-products per multiply on the
// bf16 MFMA (conv1_bf16x3.hip) when the plan says so, else the fp32 MFMA (conv_rowwin.hip) -- same tiles, same window, same output
// addressing, other operands.  out = [B][Ho][Wo][cs_out], channels c_off .. c_off + N; tickets != NULL: the launch zeroes them.
static int conv1_rowwin(vstab_ctx *ctx, bool bf16x3, const float *feats, int B, int H, int W, int Cin, int Ho, int Wo, int N, int Npad,
                        float *out, int cs_out, int c_off, unsigned *tickets, hipStream_t stream, hipEvent_t ev_a, hipEvent_t ev_b,
                        const char **kname, bool *launched)
{
    const Layer &e = NET[0];
    const float *dw = ctx->dev_weights;
    *launched = false;
    RowWinDesc d = rowwin_desc(B, H, W, Cin, e.k, e.s, e.p, Ho, Wo, N, Npad, cs_out, c_off, 1);
    if (!d.ok || ((uintptr_t)feats & 15) != 0) return VSTAB_OK;
    const bool b3 = bf16x3 && ctx->enc0_b3 != 0 && conv1_bf16x3_geometry_ok(d.main);
    RowWinParams &r = d.main, &t = d.tail;
    r.in = t.in = feats; r.out = t.out = out; r.bias = t.bias = dw + ctx->enc_b[0];
    r.wpk = t.wpk = dw + (b3 ? ctx->enc0_b3 : ctx->enc0_rw);
    auto launch1 = [&](const RowWinParams &q, hipEvent_t a, hipEvent_t b) {
        return b3 ? launch_conv1_bf16x3(q, stream, a, b) : launch_conv_rowwin(q, stream, a, b);
    };
    if (tickets) { r.clear_words = tickets; r.clear_n = SKINNY_MAX_TILES; }
    *launched = true;
    if (d.two) {
        // 128 k + (1..64) columns: k full tiles, then the rest as ONE 64-pixel tile (second launch; events span both)
        HIP_TRY(ctx, launch1(r, ev_a, nullptr));
        HIP_TRY(ctx, launch1(t, nullptr, ev_b));
        *kname = b3 ? "conv1_bf16x3_kernel<7, 2> + <4, 1> tail" : "conv_rowwin_kernel<7, 2> + <4, 1> tail";
        return VSTAB_OK;
    }
    HIP_TRY(ctx, launch1(r, ev_a, ev_b));
    if (b3) *kname = r.MB == 2 ? "conv1_bf16x3_kernel<7, 2>" : "conv1_bf16x3_kernel<4, 1>";
    else *kname = r.MB == 2 ? "conv_rowwin_kernel<7, 2>" : "conv_rowwin_kernel<4, 1>";
    return VSTAB_OK;
}

// conv1 alone (diagnostic: tests of the layer's two forms), as the forward of this context would run it
extern "C" int vstab_conv1_forward(vstab_ctx *ctx, const float *feats, int B, int H, int W, int Cin, float *out, int cs_out, int c_off,
                                   void *stream_)
{
    if (!ctx) return fail(nullptr, VSTAB_E_STATE, "conv1_forward: ctx is NULL");
    if (!ctx->loaded) return fail(ctx, VSTAB_E_STATE, "conv1_forward: vstab_load_weights has not been called");
    if (Cin != ctx->cin) return fail(ctx, VSTAB_E_SHAPE, "conv1_forward: feats has %d channels, weights expect %d", Cin, ctx->cin);
    if (!feats || !out) return fail(ctx, VSTAB_E_STATE, "conv1_forward: NULL buffer");
    const PlanPin pin = pin_of(ctx);
    std::unique_ptr<Plan> pl(new (std::nothrow) Plan);
    if (!pl) return fail(ctx, VSTAB_E_NOMEM, "conv1_forward: out of host memory");
    if (B < 1 || !make_plan(B, H, W, Cin, *pl, &pin)) return fail(ctx, VSTAB_E_SHAPE, "conv1_forward: unsupported problem %dx%dx%dx%d", B, H, W, Cin);
    const ConvParams &p = pl->cp[0];
    if (c_off < 0 || cs_out < c_off + p.N || (long long)B * p.Ho * p.Wo * cs_out * 4 >= 0x80000000LL)
        return fail(ctx, VSTAB_E_SHAPE, "conv1_forward: output slice %d + %d of %d channels", c_off, p.N, cs_out);
    if (((uintptr_t)feats & 15) || ((uintptr_t)out & 3)) return fail(ctx, VSTAB_E_ALIGN, "conv1_forward: feats must be 16-byte aligned");
    const char *kname = nullptr;
    bool launched = false;
    const int rc = conv1_rowwin(ctx, pl->conv1_bf16x3, feats, B, H, W, Cin, p.Ho, p.Wo, p.N, p.Npad, out, cs_out, c_off, nullptr,
                                (hipStream_t)stream_, nullptr, nullptr, &kname, &launched);
    if (rc != VSTAB_OK) return rc;
    if (!launched) return fail(ctx, VSTAB_E_SHAPE, "conv1_forward: the row-window kernels do not take this geometry");
    return VSTAB_OK;
}

static int forward_chunk(vstab_ctx *ctx, const float *feats, int B, int H, int W, int Cin, float *pf6, float *pf5,
                         float *pf4, float *pf3, float *pf2, void *workspace, size_t workspace_bytes, void *stream_, FusedTail *tail)
{
    Plan pl;
    const PlanPin pin = pin_of(ctx);
    if (!make_plan(B, H, W, Cin, pl, &pin)) return fail(ctx, VSTAB_E_SHAPE, "forward: unsupported problem %dx%dx%dx%d", B, H, W, Cin);
    if (workspace_bytes < pl.total) return fail(ctx, VSTAB_E_NOMEM, "forward: workspace %zu < %zu bytes", workspace_bytes, pl.total);
    if (((uintptr_t)workspace & 255) != 0) return fail(ctx, VSTAB_E_ALIGN, "forward: workspace must be 256-byte aligned");
    if (((uintptr_t)feats & 15) || ((uintptr_t)pf6 & 7) || ((uintptr_t)pf5 & 7) || ((uintptr_t)pf4 & 7) ||
        ((uintptr_t)pf3 & 7) || ((uintptr_t)pf2 & 7))
        return fail(ctx, VSTAB_E_ALIGN, "forward: feats must be 16-byte and flows 8-byte aligned");
    hipStream_t stream = (hipStream_t)stream_;
    char *ws = (char *)workspace;
    auto buf = [&](int b) { return (float *)(ws + pl.off[b]); };
    const float *dw = ctx->dev_weights;
    // the weight-stream layers finish their split-K inside the launch by tickets (conv_skinny.hip).  The words live in THIS workspace and
    // are zeroed here: a launch leaves them zero, but the workspace is the caller's (first use, reuse of freed memory) and a launch that
    // failed mid-flight leaves them dirty
    unsigned *tickets = reinterpret_cast<unsigned *>(buf(B_TICKETS));
    bool any_tickets = false;
    for (int i = 0; i < 14; ++i) any_tickets = any_tickets || (pl.skinny[i] && pl.cp[i].ksplit > 1);
    bool tickets_cleared = !any_tickets;          // the first layer's launch clears them when it is the row-window kernel; else a memset node

    // optional per-launch events
    hipEvent_t *ev = nullptr;
    if (ctx->prof) {
        const size_t need = (size_t)(ctx->prof_forwards + 1) * 30;
        while (ctx->prof_ev.size() < need) {
            hipEvent_t e;
            HIP_TRY(ctx, hipEventCreate(&e));
            ctx->prof_ev.push_back(e);
        }
        ev = ctx->prof_ev.data() + (size_t)ctx->prof_forwards * 30;
        for (int i = 0; i < 15; ++i) {
            const ConvParams &p = pl.cp[i];
            double mac = 0;
            if (i < 10 && pl.wino[i]) mac = 16.0 * pl.wcp[i].Mmax * NET[i].cin * p.N;      // MACs the Winograd-domain GEMM issues (4/9 of direct)
            else if (i < 10) mac = (double)p.ph[0].M * NET[i].k * NET[i].k * (i == 0 ? Cin : NET[i].cin) * p.N;
            else if (i < 14 && pl.wdec[i - 10]) {                          // MACs the 9-position GEMM issues (9/16 of direct, plus the ragged tile grid)
                for (int k = 0; k < 9; ++k) mac += (double)pl.wdcp[i - 10].ph[k].M * NET[i].cin * 4.0 * p.N;
            }
            else if (i < 14) mac = (double)B * p.Ho * p.Wo * 4.0 * NET[i].cin * p.N;
            else mac = (double)p.ph[0].M * 194.0 * 18.0;
            ctx->prof_flops[i] += 2.0 * mac;
            double dmac = mac;                           // the same layer as a direct convolution (SURVEY.md 8d's accounting)
            if (i < 10 && pl.wino[i]) dmac = (double)p.ph[0].M * 9.0 * NET[i].cin * p.N;
            if (i >= 10 && i < 14 && pl.wdec[i - 10]) dmac = (double)B * p.Ho * p.Wo * 4.0 * NET[i].cin * p.N;
            ctx->prof_flops_direct[i] += 2.0 * dmac;
        }
    }
    // (the context is written only while profiling: plain forwards on one context may be issued from several host threads)
#define PROF_NAME(slot, name) do { if (ev) ctx->prof_kernel[slot] = (name); } while (0)
#define EV_A(slot) (ev ? ev[2 * (slot)] : nullptr)
#define EV_B(slot) (ev ? ev[2 * (slot) + 1] : nullptr)

    static const char *const HEAD_RANGE[4] = {"predict_flow6+upsample6_5", "predict_flow5+upsample5_4", "predict_flow4+upsample4_3", "predict_flow3+upsample3_2"};
    TraceRange whole_range("flownetS_pyramid");
    // encoder (model.py:807-844)
    for (int i = 0; i < 10; ++i) {
        const Layer &e = NET[i];
        TraceRange layer_range(e.name);
        ConvParams p = pl.cp[i];
        if (i == 0) {           // first layer: row-window kernel when its alignment conditions hold
            const char *kname = nullptr;
            bool launched = false;
            const int rc = conv1_rowwin(ctx, pl.conv1_bf16x3, feats, B, H, W, Cin, p.Ho, p.Wo, p.N, p.Npad, buf(B_CONV1), p.Cs_out, 0,
                                        tickets_cleared ? nullptr : tickets, stream, EV_A(0), EV_B(0), &kname, &launched);
            if (rc != VSTAB_OK) return rc;
            if (launched) { tickets_cleared = true; PROF_NAME(0, kname); continue; }
        }
        if (!tickets_cleared) { HIP_TRY(ctx, hipMemsetAsync(tickets, 0, pl.bytes[B_TICKETS], stream)); tickets_cleared = true; }
        if (pl.wino[i]) {       // transform, 16-position GEMM on the MFMA kernel, inverse transform (+ bias, leaky relu)
            ConvParams q = pl.wcp[i];
            const int cin_i = e.cin;
            HIP_TRY(ctx, launch_wino_input(buf(e.in), B, pl.eh[i], pl.ew[i], in_buf(e).cs, 0, cin_i, buf(B_WINO_V), stream));
            q.in = buf(B_WINO_V); q.out = buf(B_WINO_M);
            q.wpk = dw + ctx->wino_w[i]; q.bias = dw + ctx->zero_b; q.partial = buf(B_PARTIAL);
            const int T_i = ((pl.eh[i] + 1) / 2) * ((pl.ew[i] + 1) / 2);
            // (VSTAB_PLAN_NO_WINO_STREAM: the tiled launch below for every stage -- the B side of the stream form's A/B, same bits)
            const int P_i = (pin.flags & VSTAB_PLAN_NO_WINO_STREAM) ? 0 : wino_gemm_stream_positions(B, T_i, cin_i, e.cout);
            if (P_i > 0) {       // streams of positions (wino_gemm_stream.hip): B=8 512x512 conv3_1 (8 positions per workgroup), conv4_1 (4)
                HIP_TRY(ctx, launch_wino_gemm_stream(q.in, q.wpk, q.out, B, T_i, cin_i, e.cout, P_i, stream, EV_A(i), EV_B(i)));
                PROF_NAME(i, "wino_gemm_stream_kernel");
            } else {
                HIP_TRY(ctx, launch_conv(q, pl.wtile[i], true, stream, EV_A(i), EV_B(i)));
                PROF_NAME(i, conv_kernel_name(pl.wtile[i], true));
            }
            HIP_TRY(ctx, launch_wino_output(buf(B_WINO_M), B, pl.eh[i], pl.ew[i], e.cout, dw + ctx->enc_b[i], 1, buf(e.out),
                                            out_buf(e).cs, 0, stream));
            continue;
        }
        p.in = e.in < 0 ? feats : buf(e.in);
        p.out = buf(e.out);
        p.wpk = dw + ctx->enc_w[i];
        p.bias = dw + ctx->enc_b[i];
        p.partial = buf(B_PARTIAL);
        if (pl.skinny[i]) {
            HIP_TRY(ctx, launch_conv_skinny(p, tickets, stream, EV_A(i), EV_B(i)));
            PROF_NAME(i, "conv_skinny_kernel<1, 4>");
            continue;
        }
        HIP_TRY(ctx, launch_conv(p, pl.tile[i], pl.vec4[i], stream, EV_A(i), EV_B(i)));
        PROF_NAME(i, conv_kernel_name(pl.tile[i], pl.vec4[i]));
    }
    // decoder (model.py:847-880)
    float *pfs[5] = {pf6, pf5, pf4, pf3, pf2};
    // One refinement level = its flow head (model.py:847-848 ...: 3x3 -> 2 conv as a tap-table GEMM whose split-K slabs stay uncombined,
    // then predict_up: slab sum, tap gather, fold with the upsampled coarser flow, upsample_flowN into the next concat's flow channels)
    // and its transposed convolution (model.py:850-851 ...).  Both read the SAME tensor and neither needs the other, so they run as
    // TWO launches instead of four: conv_dual_kernel (deconv tiles + tap-table tiles side by side), then combine_predict_up_kernel
    // (the deconv's split-K combine + predict_up side by side).  For one sample every one of the four was little more than a
    // launch's fixed latency.  VSTAB_PLAN_NO_DUAL restores the four-launch sequence (A/B; same arithmetic, same bits).
    for (int l = 0; l < 4; ++l) {
        const float *prev = l == 0 ? nullptr : pfs[l - 1];
        const Layer &d = dec_layer(l);
        const int ph_ = l == 0 ? 0 : pl.eh[LVL_ENC[l - 1]], pw_ = l == 0 ? 0 : pl.ew[LVL_ENC[l - 1]];      // the coarser level's size
        const int oh = pl.eh[LVL_ENC[l + 1]], ow = pl.ew[LVL_ENC[l + 1]];                                  // the finer level the flow is upsampled to
        ConvParams pd = pl.cp[10 + l], pt = pl.cp[15 + l];
        pd.in = buf(d.in); pd.out = buf(d.out);
        pd.wpk = dw + ctx->dec_w[l]; pd.bias = dw + ctx->dec_b[l]; pd.partial = buf(B_PARTIAL);
        const size_t dec_slab = pd.ksplit > 1 ? (size_t)pd.nphase * pd.ksplit * pd.Mmax * pd.Npad : 0;   // the tap table's slabs sit behind the deconv's
        pt.in = buf(head_layer(l).in); pt.out = buf(head_layer(l).out);
        pt.wpk = dw + ctx->pred_w[l]; pt.bias = dw + ctx->tab_b; pt.partial = buf(B_PARTIAL) + dec_slab;
        const float *tsrc = pt.ksplit > 1 ? pt.partial : pt.out;
        const bool fuse = !(pin.flags & VSTAB_PLAN_NO_DUAL) && !pl.skinny[10 + l];
        // the level's head: predict_up over the tap table (optionally with the transposed convolution's combine / inverse transform)
        auto head = [&](const float *taps, const ConvParams *combine, const WdecOutArgs *wdec) {
            return launch_predict_up(taps, pt.ksplit, (long long)pt.Mmax * pt.Npad, B, pt.Hi, pt.Wi, dw + ctx->pred_b[l], prev, ph_, pw_, pfs[l],
                                     ctx->up[l], buf(d.out), oh, ow, out_buf(d).cs, out_buf(d).c - 2, stream, combine, wdec);
        };
        // problem `a` beside the tap-table tiles in ONE launch; a tile shape the two-problem kernel is not built for: one launch each
        // (slabs uncombined either way: the combine rides with predict_up)
        auto dual = [&](const ConvParams &a, ConvTile ta) -> int {
            const hipError_t e = launch_conv_dual(a, ta, pt, pl.tile[15 + l], stream, EV_A(10 + l), EV_B(10 + l));
            if (e == hipErrorNotSupported) {
                HIP_TRY(ctx, launch_conv(pt, pl.tile[15 + l], true, stream, nullptr, nullptr, false));
                HIP_TRY(ctx, launch_conv(a, ta, true, stream, EV_A(10 + l), EV_B(10 + l), false));
                PROF_NAME(10 + l, conv_kernel_name(ta, true));
            } else {
                HIP_TRY(ctx, e);
                PROF_NAME(10 + l, dual_kernel_name(ta));
            }
            return VSTAB_OK;
        };
        if (fuse && pl.wdec[l]) {
            // Winograd F(2x2,2x2): input transform, the 9-position GEMM beside the level's tap-table tiles, inverse transform (+ bias, leaky
            // relu) into the concat slice; predict_up has no slabs of the transposed convolution to sum
            const WdecGeom &g = pl.wdg[l];
            {
                TraceRange r2(d.name);
                HIP_TRY(ctx, launch_wdec_input(pd.in, B, pd.Hi, pd.Wi, pd.Cs_in, buf(B_WINO_V), g, stream));
                ConvParams q = pl.wdcp[l];
                q.in = buf(B_WINO_V); q.out = buf(B_WINO_M); q.wpk = dw + ctx->wdec_w[l]; q.bias = dw + ctx->zero_b; q.partial = buf(B_PARTIAL);
                pt.partial = buf(B_PARTIAL);
                if (const int rc = dual(q, pl.wdtile[l])) return rc;
            }
            // the inverse transform (+ bias, leaky relu) shares its launch with predict_up: different channel slices of the same concat
            TraceRange r3(HEAD_RANGE[l]);
            const WdecOutArgs wo{buf(B_WINO_M), pd.N / 4, dw + ctx->dec_b[l], 1, buf(d.out), pd.Ho, pd.Wo, pd.Cs_out, pd.c_off, g};
            HIP_TRY(ctx, head(pt.ksplit > 1 ? pt.partial : pt.out, nullptr, &wo));
            continue;
        }
        if (fuse) {
            {
                TraceRange r2(d.name);
                if (const int rc = dual(pd, pl.tile[10 + l])) return rc;
            }
            TraceRange r3(HEAD_RANGE[l]);
            HIP_TRY(ctx, head(tsrc, &pd, nullptr));
            continue;
        }
        {
            TraceRange head_range(HEAD_RANGE[l]);
            HIP_TRY(ctx, launch_conv(pt, pl.tile[15 + l], true, stream, nullptr, nullptr, false));
            HIP_TRY(ctx, head(tsrc, nullptr, nullptr));
        }
        TraceRange layer_range(d.name);
        if (pl.skinny[10 + l]) {
            HIP_TRY(ctx, launch_conv_skinny(pd, tickets, stream, EV_A(10 + l), EV_B(10 + l)));
            PROF_NAME(10 + l, "conv_skinny_kernel<1, 4>");
        } else {
            HIP_TRY(ctx, launch_conv(pd, pl.tile[10 + l], true, stream, EV_A(10 + l), EV_B(10 + l)));
            PROF_NAME(10 + l, conv_kernel_name(pl.tile[10 + l], true));
        }
    }
    // full-resolution head (model.py:882-887)
    {
        TraceRange layer_range("predict_flow2");
        ConvParams p = pl.cp[14];
        p.in = buf(B_CONCAT2); p.out = buf(B_T);
        const long long M2 = (long long)B * pl.eh[1] * pl.ew[1];
        if (!tap_panel_applicable(M2, p.Cs_in, p.in, p.out)) return fail(ctx, VSTAB_E_SHAPE, "predict_flow2 tap table: unsupported geometry");
        HIP_TRY(ctx, launch_tap_panel(p.in, M2, dw + ctx->tab_wp, p.out, stream, EV_A(14), EV_B(14)));
        PROF_NAME(14, "tap_panel_kernel");
        hipError_t te = hipErrorNotSupported;
        if (tail && !(pin.flags & VSTAB_PLAN_NO_TAIL)) {       // gather + glue + warp of this chunk's frames in one launch, when the geometry allows
            TraceRange tail_range("predict_flow2 gather+flow_glue+tf_warp");
            if (tail->frame8)
                te = launch_pf2_glue_warp_u8(buf(B_T), B, pl.eh[1], pl.ew[1], dw + ctx->pred2_b, pf3, pl.eh[3], pl.ew[3], pf2, H, W, tail->frame8,
                                             tail->outflow, tail->out8, tail->oh, tail->ow, stream);
            else
                te = launch_pf2_glue_warp(buf(B_T), B, pl.eh[1], pl.ew[1], dw + ctx->pred2_b, pf3, pl.eh[3], pl.ew[3], pf2, H, W, tail->frame,
                                          tail->outflow, tail->warped, tail->oh, tail->ow, stream);
            if (te != hipSuccess && te != hipErrorNotSupported) HIP_TRY(ctx, te);
            tail->fused = te == hipSuccess;
        }
        if (te != hipSuccess) HIP_TRY(ctx, launch_pf2(buf(B_T), B, pl.eh[1], pl.ew[1], dw + ctx->pred2_b, pf3, pl.eh[3], pl.ew[3], pf2, H, W, stream));
    }
#undef EV_A
#undef EV_B
#undef PROF_NAME
    if (ev) ctx->prof_forwards++;
    return VSTAB_OK;
}

// (string literals: the profiler's name slots are plain pointers, nothing a forward does allocates)
static const char *conv_kernel_name(ConvTile t, bool vec4)
{
    const bool dma = conv_uses_lds_dma(t, vec4);
#define VSTAB_KN(shape) (vec4 ? (dma ? "conv_mfma_kernel<" shape ", true, true>" : "conv_mfma_kernel<" shape ", true, false>") \
                              : (dma ? "conv_mfma_kernel<" shape ", false, true>" : "conv_mfma_kernel<" shape ", false, false>"))
    switch (t) {
    case TILE_128x128: return VSTAB_KN("128, 128, 2, 2");
    case TILE_128x64: return VSTAB_KN("128, 64, 2, 2");
    case TILE_64x128: return VSTAB_KN("64, 128, 1, 4");
    case TILE_64x64: return VSTAB_KN("64, 64, 2, 2");
    case TILE_256x32: return VSTAB_KN("256, 32, 4, 1");
    default: return VSTAB_KN("128, 32, 4, 1");
    }
#undef VSTAB_KN
}

static const char *dual_kernel_name(ConvTile t)
{
    const bool dma = conv_uses_lds_dma(t, true);
#define VSTAB_DN(shape) (dma ? "conv_dual_kernel: conv_mfma_kernel<" shape ", true, true> + <128, 32> tap table" \
                             : "conv_dual_kernel: conv_mfma_kernel<" shape ", true, false> + <128, 32> tap table")
    switch (t) {
    case TILE_128x128: return VSTAB_DN("128, 128, 2, 2");
    case TILE_128x64: return VSTAB_DN("128, 64, 2, 2");
    case TILE_64x128: return VSTAB_DN("64, 128, 1, 4");
    case TILE_64x64: return VSTAB_DN("64, 64, 2, 2");
    case TILE_256x32: return VSTAB_DN("256, 32, 4, 1");
    default: return VSTAB_DN("128, 32, 4, 1");
    }
#undef VSTAB_DN
}

// ------------------------------------------------------------------------- profiling
extern "C" int vstab_profile_kernel_name(vstab_ctx *ctx, int slot, char *buf, int cap)
{
    if (!ctx || !buf || cap < 1 || slot < 0 || slot > 14) return fail(ctx, VSTAB_E_STATE, "profile_kernel_name: bad argument");
    std::snprintf(buf, (size_t)cap, "%s", ctx->prof_kernel[slot] ? ctx->prof_kernel[slot] : "");
    return VSTAB_OK;
}

extern "C" int vstab_profile_enable(vstab_ctx *ctx, int enable)
{
    if (!ctx) return fail(nullptr, VSTAB_E_STATE, "profile_enable: ctx is NULL");
    ctx->prof = enable != 0;
    return VSTAB_OK;
}

extern "C" int vstab_profile_reset(vstab_ctx *ctx)
{
    if (!ctx) return fail(nullptr, VSTAB_E_STATE, "profile_reset: ctx is NULL");
    ctx->prof_forwards = 0;
    for (double &f : ctx->prof_flops) f = 0;
    for (double &f : ctx->prof_flops_direct) f = 0;
    return VSTAB_OK;
}

extern "C" int vstab_profile_read(vstab_ctx *ctx, double *ms_sum15, double *flops15, int *n_forwards)
{
    if (!ctx || !ms_sum15 || !flops15 || !n_forwards) return fail(ctx, VSTAB_E_STATE, "profile_read: NULL argument");
    for (int i = 0; i < 15; ++i) { ms_sum15[i] = 0; flops15[i] = ctx->prof_flops[i]; }
    for (int f = 0; f < ctx->prof_forwards; ++f)
        for (int i = 0; i < 15; ++i) {
            float ms = 0.f;
            HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->prof_ev[(size_t)f * 30 + 2 * i], ctx->prof_ev[(size_t)f * 30 + 2 * i + 1]));
            ms_sum15[i] += ms;
        }
    *n_forwards = ctx->prof_forwards;
    return VSTAB_OK;
}

extern "C" int vstab_profile_read_direct(vstab_ctx *ctx, double *flops15)
{
    if (!ctx || !flops15) return fail(ctx, VSTAB_E_STATE, "profile_read_direct: NULL argument");
    for (int i = 0; i < 15; ++i) flops15[i] = ctx->prof_flops_direct[i];
    return VSTAB_OK;
}

// ------------------------------------------------------------------------- the network + the evaluator's tail
// evaluate_originalSize's whole graph (main:491-514) behind ONE call: the network, then the flow glue + tf_warp launch.
extern "C" int vstab_stabilise_originalsize(vstab_ctx *ctx, const float *feats, int B, int H, int W, int Cin, const float *frame, int oh,
                                            int ow, float *pf6, float *pf5, float *pf4, float *pf3, float *pf2, float *outflow,
                                            float *warped, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!frame || !warped) return fail(ctx, VSTAB_E_STATE, "stabilise_originalsize: NULL buffer");
    if (oh < 1 || ow < 1) return fail(ctx, VSTAB_E_SHAPE, "stabilise_originalsize: bad output size");
    // the tail (predict_flow2's gather, the glue, tf_warp) rides in the forward's last launch when its geometry allows (flow_ops.hip)
    FusedTail tail{frame, outflow, warped, oh, ow, false, nullptr, nullptr};
    const bool try_fused = (((uintptr_t)frame | (uintptr_t)warped | (uintptr_t)outflow) & 15) == 0;
    const int rc = forward_impl(ctx, feats, B, H, W, Cin, pf6, pf5, pf4, pf3, pf2, workspace, workspace_bytes, stream, try_fused ? &tail : nullptr);
    if (rc != VSTAB_OK) return rc;
    if (tail.fused) return VSTAB_OK;
    const int rc2 = vstab_flow_glue_warp(pf2, B, H - 2, W - 2, frame, outflow, warped, oh, ow, 3, H, W, stream);
    if (rc2 != VSTAB_OK) adopt_last_error(ctx);
    return rc2;
}

// One frame of the evaluator's loop (main:550-558, 568-569, 497-514, 625/630, 556) as ONE call: network input from the history slots + the
// frame (cv2.resize inside the launch), the network, the 8-bit glue + warp launch, the stabilised frame resized into its history slot.
extern "C" int vstab_clip_step(vstab_ctx *ctx, const uint8_t *const *slots8, const uint8_t *frame, int n, int net_h, int net_w, int oh, int ow,
                               float *feats, float *pf6, float *pf5, float *pf4, float *pf3, float *pf2, float *outflow, uint8_t *out,
                               uint8_t *ring_slot, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!ctx) return fail(nullptr, VSTAB_E_STATE, "clip_step: ctx is NULL");
    if (!slots8 || !frame || !feats || !out || !ring_slot) return fail(ctx, VSTAB_E_STATE, "clip_step: NULL buffer");
    if (n < 1 || net_h < 3 || net_w < 4 || oh < 1 || ow < 1) return fail(ctx, VSTAB_E_SHAPE, "clip_step: bad shape");
    {   // the warp GATHERS frame pixels while other workgroups already write `out`, and the history slot is resized from `out`:
        // neither may overlap the frame, nor each other
        const size_t fb = (size_t)n * oh * ow * 3, sb = (size_t)n * net_h * net_w * 3;
        auto overlap = [](const void *a, size_t na, const void *b, size_t nb) {
            const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
            return x < y + nb && y < x + na;
        };
        if (overlap(out, fb, frame, fb) || overlap(ring_slot, sb, frame, fb) || overlap(ring_slot, sb, out, fb))
            return fail(ctx, VSTAB_E_STATE, "clip_step: out / ring_slot / frame must not overlap");
    }
    int rc = vstab_assemble_input_resized(slots8, frame, n, net_h, net_w, oh, ow, feats, stream);
    // the network; its last launch also does the 8-bit glue + warp of the frame when the geometry allows (flow_ops.hip, pf2_glue_warp_kernel)
    FusedTail tail{nullptr, outflow, nullptr, oh, ow, false, frame, out};
    const bool try_fused = (((uintptr_t)outflow & 7) | ((uintptr_t)out & 3)) == 0 && (long long)n * oh * ow < (1ll << 31) / 3;
    if (rc == VSTAB_OK) rc = forward_impl(ctx, feats, n, net_h, net_w, 27, pf6, pf5, pf4, pf3, pf2, workspace, workspace_bytes, stream, try_fused ? &tail : nullptr);
    else adopt_last_error(ctx);
    if (rc != VSTAB_OK) return rc;
    if (!tail.fused) rc = vstab_flow_glue_warp_u8(pf2, n, net_h - 2, net_w - 2, frame, outflow, out, oh, ow, net_h, net_w, stream);
    if (rc == VSTAB_OK) rc = vstab_resize_u8(out, n, oh, ow, ring_slot, net_h, net_w, stream);
    if (rc != VSTAB_OK) adopt_last_error(ctx);
    return rc;
}
