// The VGG16 trunk's layer table and launch plan, shared by its forward (vgg_api.cpp) and its backward (vgg_grad_api.cpp).
#pragma once
#include <cstddef>

struct vstab_ctx;

struct VggLayer { const char *name; int cin, cout; bool pool_after; };
extern const VggLayer VGG[13];

struct VggPlan { int h[18], w[18], c[18]; size_t partial_floats, wino_v, wino_m; bool wino[13]; };
bool vgg_plan(int B, int H, int W, VggPlan &v);
int vgg_max_chunk(int B, int H, int W);         // largest batch whose every tensor stays below 2 GiB
void vgg_backward_free(vstab_ctx *ctx);         // drops the transposed-Winograd operands the backward keeps on the context
