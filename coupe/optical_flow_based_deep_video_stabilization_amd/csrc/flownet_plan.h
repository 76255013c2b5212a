// The FlowNetS pyramid (model.py:786-893) as ONE table of its 19 conv-like launches and one of its workspace buffers, and the launch
// plan made from them (flownet_plan.cpp).  The weight loader, the forward schedule and the host-plan views all read these tables.
#pragma once
#include "api_internal.h"
#include "conv_desc.h"

enum Buf { B_CONV1, B_CONCAT2, B_CONV3, B_CONCAT3, B_CONV4, B_CONCAT4, B_CONV5, B_CONCAT5, B_CONV6, B_CONV6_1, B_T,
           B_T6, B_T5, B_T4, B_T3, B_TICKETS, B_PARTIAL, B_WINO_V, B_WINO_M, N_BUF };
// B_PARTIAL, B_WINO_V, B_WINO_M stay LAST: their sizes depend on plan decisions (split-K factors, Winograd or direct) that a pinned
// plan may change, while every offset before them depends on the shape alone (vstab_workspace_layout relies on it)
static_assert(B_PARTIAL == N_BUF - 3 && B_WINO_V == N_BUF - 2 && B_WINO_M == N_BUF - 1, "plan-dependent buffers must come last");

// [B][h][w][cs] with the size of encoder stage `level` and c used channels; level < 0: a flat run of words sized by the plan
struct BufSpec { const char *name; int level, c, cs; };
constexpr BufSpec BUFS[N_BUF] = {
    {"conv1", 0, 64, 64},         {"concat2", 1, 194, 196},   {"conv3", 2, 256, 256},     {"concat3", 3, 386, 388},
    {"conv4", 4, 512, 512},       {"concat4", 5, 770, 772},   {"conv5", 6, 512, 512},     {"concat5", 7, 1026, 1028},
    {"conv6", 8, 1024, 1024},     {"conv6_1", 9, 1024, 1024}, {"pf2_taps", 1, 32, 32},    {"pf6_taps", 9, 32, 32},
    {"pf5_taps", 7, 32, 32},      {"pf4_taps", 5, 32, 32},    {"pf3_taps", 3, 32, 32},    {"tickets", -1, 0, 0},
    {"splitk", -1, 0, 0},         {"winograd_in", -1, 0, 0},  {"winograd_out", -1, 0, 0}};

// rows 0-9 the encoder (variables "<name + 4>/..."), 10-13 the refinement levels' 4x4 stride-2 transposed convs (level l = row - 10),
// 14 predict_flow2's tap table, 15-18 those of predict_flow6..3 (3x3 -> 2 heads as 1x1 GEMMs with 18, padded 32, columns over the
// whole pixel).  cin = channels the filter has (0: the caller's); `in` < 0: the network input; c_off = first output channel.
enum LayerKind { L_CONV, L_DECONV, L_TAPS };
struct Layer { const char *name; LayerKind kind; int k, s, p, cin, cout, in, out, c_off; };
constexpr int N_LAYER = 19;
constexpr Layer NET[N_LAYER] = {
    {"conv1", L_CONV, 7, 2, 3, 0, 64, -1, B_CONV1, 0},              {"conv2", L_CONV, 5, 2, 2, 64, 128, B_CONV1, B_CONCAT2, 0},
    {"conv3", L_CONV, 5, 2, 2, 128, 256, B_CONCAT2, B_CONV3, 0},    {"conv3_1", L_CONV, 3, 1, 1, 256, 256, B_CONV3, B_CONCAT3, 0},
    {"conv4", L_CONV, 3, 2, 1, 256, 512, B_CONCAT3, B_CONV4, 0},    {"conv4_1", L_CONV, 3, 1, 1, 512, 512, B_CONV4, B_CONCAT4, 0},
    {"conv5", L_CONV, 3, 2, 1, 512, 512, B_CONCAT4, B_CONV5, 0},    {"conv5_1", L_CONV, 3, 1, 1, 512, 512, B_CONV5, B_CONCAT5, 0},
    {"conv6", L_CONV, 3, 2, 1, 512, 1024, B_CONCAT5, B_CONV6, 0},   {"conv6_1", L_CONV, 3, 1, 1, 1024, 1024, B_CONV6, B_CONV6_1, 0},
    {"deconv5", L_DECONV, 4, 2, 1, 1024, 512, B_CONV6_1, B_CONCAT5, 512}, {"deconv4", L_DECONV, 4, 2, 1, 1026, 256, B_CONCAT5, B_CONCAT4, 512},
    {"deconv3", L_DECONV, 4, 2, 1, 770, 128, B_CONCAT4, B_CONCAT3, 256},  {"deconv2", L_DECONV, 4, 2, 1, 386, 64, B_CONCAT3, B_CONCAT2, 128},
    {"predict2", L_TAPS, 3, 1, 1, 194, 2, B_CONCAT2, B_T, 0},       {"predict6", L_TAPS, 3, 1, 1, 1024, 2, B_CONV6_1, B_T6, 0},
    {"predict5", L_TAPS, 3, 1, 1, 1026, 2, B_CONCAT5, B_T5, 0},     {"predict4", L_TAPS, 3, 1, 1, 770, 2, B_CONCAT4, B_T4, 0},
    {"predict3", L_TAPS, 3, 1, 1, 386, 2, B_CONCAT3, B_T3, 0}};
constexpr int LVL_ENC[5] = {9, 7, 5, 3, 1};                 // encoder stage that gives refinement level 6..2 its size
constexpr const Layer &dec_layer(int l) { return NET[10 + l]; }
constexpr const Layer &head_layer(int l) { return NET[15 + l]; }     // predict6,5,4,3
constexpr const BufSpec &in_buf(const Layer &L) { return BUFS[L.in]; }
constexpr const BufSpec &out_buf(const Layer &L) { return BUFS[L.out]; }

constexpr bool net_is_consistent()
{
    for (int i = 1; i < 10; ++i)           // an encoder stage reads the first channels of what the previous one wrote, skip first
        if (NET[i].in != NET[i - 1].out || NET[i].cin != NET[i - 1].cout || NET[i].cout > out_buf(NET[i]).c) return false;
    for (int i = 10; i < N_LAYER; ++i)     // the decoder's launches consume whole (concat) tensors
        if (NET[i].cin != in_buf(NET[i]).c) return false;
    for (int l = 0; l < 4; ++l) {          // concat = [skip | deconv | 2 flow channels]; the level's head reads what its deconv reads
        const Layer &d = dec_layer(l);
        if (d.c_off + d.cout + 2 != out_buf(d).c || head_layer(l).in != d.in) return false;
        if (BUFS[d.out].level != LVL_ENC[l + 1] || BUFS[d.in].level != LVL_ENC[l] || BUFS[head_layer(l).out].level != LVL_ENC[l]) return false;
    }
    for (int b = 0; b < N_BUF; ++b)
        if (BUFS[b].cs < BUFS[b].c || (BUFS[b].cs & 3)) return false;
    return NET[14].in == dec_layer(3).out;
}
static_assert(net_is_consistent(), "NET and BUFS disagree");

struct Plan {
    int B, H, W, Cin;
    int eh[10], ew[10];
    size_t off[N_BUF];      // byte offsets
    size_t bytes[N_BUF];
    size_t total;
    // conv-like launches, one per row of NET
    vstab::ConvParams cp[N_LAYER];
    vstab::ConvTile tile[N_LAYER];
    bool vec4[N_LAYER];
    bool conv1_bf16x3;      // the first layer's products as six bf16 piece-products on the bf16 MFMA (conv1_bf16x3.hip) when its row-window
                            // conditions hold at launch time; false: the fp32 MFMA (VSTAB_PLAN_CONV1_FP32, or a filter the form is not built for)
    bool skinny[N_LAYER];   // few-row layers as weight streams (conv_skinny.hip): tile[i] == TILE_SKINNY, cp[i].ksplit = its own factor
    // Winograd F(2x2,3x3) form of the 3x3 stride-1 encoder stages (cp[i] stays the direct form: host-plan tests, fallback)
    bool wino[10];
    vstab::ConvParams wcp[10];
    vstab::ConvTile wtile[10];
    // Winograd F(2x2,2x2) form of the transposed convolutions (winograd_ops.hip; cp[10 + l] stays the direct form): the 9-position GEMM
    bool wdec[4];
    vstab::ConvParams wdcp[4];
    vstab::ConvTile wdtile[4];
    vstab::WdecGeom wdg[4];
    int buf_h(int b) const { return BUFS[b].level < 0 ? 0 : eh[BUFS[b].level]; }
    int buf_w(int b) const { return BUFS[b].level < 0 ? 0 : ew[BUFS[b].level]; }
};

// What a context pins about its launch plans (vstab_set_plan_batch / vstab_set_plan_flags).  batch > 0: every per-layer decision that
// changes the ARITHMETIC of a sample -- split-K factors, Winograd or direct form, weight-stream or tiled kernel -- is taken for a
// batch of `batch` samples and reused for any smaller batch, so a sample's results do not depend on what it is batched with
// (sharded clips with ragged tails: main:553-558's samples are independent).
struct PlanPin { int batch = 0; unsigned flags = 0; };
inline PlanPin pin_of(const vstab_ctx *ctx)
{
    PlanPin pin;
    if (ctx) { pin.batch = ctx->plan_batch; pin.flags = ctx->plan_flags; }
    return pin;
}

bool level_sizes(int H, int W, int *eh, int *ew);
// allocation-free unless a pinned batch needs its reference plan
bool make_plan(int B, int H, int W, int Cin, Plan &pl, const PlanPin *pin = nullptr);
// chunk size the forward processes a batch of B in: every tensor below 2 GiB, chunks equalised; under a pinned plan batch the
// chunk size of THAT batch (ragged chunks then share its decisions).  0: one sample does not fit.
int chunk_size(const PlanPin &pin, int B, int H, int W, int Cin);
