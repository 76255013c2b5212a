// The NLDF head's geometry, workspace plan and per-context state, shared by its forward (nldf_api.cpp) and its backward
// (nldf_grad_api.cpp).
#pragma once
#include <cstddef>

namespace nldf {

constexpr int FEA = 128;                      // fea_dim, NLDF.py:33
constexpr int POOL_C[5] = {64, 128, 256, 512, 512};        // pool1..pool5 channels
constexpr int POOL_HW[5] = {176, 88, 44, 22, 11};
// concat buffers: cat_k = [Fea_Pk | Fea_Pk_LC | Fea_P(k+1)_Up]  (NLDF.py:57-66)
constexpr int CAT_C[5] = {768, 640, 512, 384, 256};        // cat1..cat5
constexpr int UP_C[4] = {512, 384, 256, 128};              // Fea_P2_Up .. Fea_P5_Up channels (into cat1..cat4)

struct NldfWeights {            // float offsets into vstab_nldf::w
    size_t g1_w, g1_b, g2_w, g2_b, g3_w, g3_b;
    size_t p_w[5], p_b[5];      // Fea_P1..P5
    size_t d_w[4], d_b[4];      // Fea_P2_Deconv .. Fea_P5_Deconv (index 0 = P2)
    size_t lf_w, lf_b, ls_w, ls_b, gs_w, gs_b;
    // every variable as given (W in the reference's layout, b), in the order of NLDF.HEAD_SHAPES: Fea_Global_1, Fea_Global_2,
    // Fea_Global, Fea_P1..P5, Fea_P5_Deconv..Fea_P2_Deconv, Local_Fea, Local_Score, Global_Score.  The backward's launchers take raw weights.
    size_t raw_w[15], raw_b[15];
};

// indices into raw_w / raw_b and into the backward's dparams30 (W at 2 i, b at 2 i + 1)
enum Layer { L_G1 = 0, L_G2 = 1, L_G = 2, L_P1 = 3, L_P5_DECONV = 8, L_P2_DECONV = 11, L_LF = 12, L_LS = 13, L_GS = 14, L_COUNT = 15 };
inline int deconv_layer(int k) { return L_P2_DECONV - k; }      // k = 0..3: the transposed conv cat(k+2) -> cat(k+1)[256:]

enum NBuf { N_G1, N_G2, N_G, N_CAT1, N_CAT2, N_CAT3, N_CAT4, N_CAT5, N_LF, N_LS, N_GS, N_PART, N_NBUF };

struct NldfPlan { size_t off[N_NBUF], bytes[N_NBUF], total; };

// [B][hw][hw][c] per NBuf entry; hw == 0: a flat run of `c` floats whatever the batch (the split-K partial sums).  The one statement
// of the workspace: nldf_plan sizes the buffers from it, vstab_nldf_workspace_layout reports it.
struct NBufSpec { const char *name; int hw, c; };
constexpr NBufSpec NBUFS[N_NBUF] = {
    {"G1", 7, FEA},        {"G2", 3, FEA},         {"Fea_Global", 1, FEA}, {"cat1", 176, 768},       {"cat2", 88, 640},
    {"cat3", 44, 512},     {"cat4", 22, 384},      {"cat5", 11, 256},      {"Local_Fea", 176, 640},  {"Local_Score", 176, 2},
    {"Global_Score", 1, 2}, {"splitk", 0, 32 << 20}};

inline bool nldf_plan(int B, NldfPlan &pl)
{
    if (B < 1 || B > 64) return false;
    size_t off = 0;
    for (int i = 0; i < N_NBUF; ++i) {
        const NBufSpec &s = NBUFS[i];
        const size_t n = s.hw ? (size_t)B * s.hw * s.hw * s.c : (size_t)s.c;
        if (n * 4 >= 0x80000000ull) return false;
        pl.off[i] = off; pl.bytes[i] = n * 4;
        off += (pl.bytes[i] + 255) / 256 * 256;
    }
    pl.total = off;
    return true;
}

}  // namespace nldf

struct vstab_nldf {             // lives inside the context (opaque to callers)
    bool loaded = false;
    float *w = nullptr;
    nldf::NldfWeights o;
};
