// Records of the optional per-launch timing of the HBM-side kernels (hbm_profile.h has the launch wrapper): host code only.
#include "hbm_profile.h"
#include <mutex>
#include <vector>

namespace vstab {
struct HbmProfState {
    std::mutex mu;
    bool on = false;
    struct Rec { hipEvent_t a, b; };
    std::vector<Rec> recs[HBM_SLOTS];
    double bytes[HBM_SLOTS] = {0};
};
static HbmProfState &hbm_prof() { static HbmProfState s; return s; }

void hbm_profile_enable(int mode)      // 0 = off (records kept), 1 = clear the records and switch on, 2 = switch on again, records kept
{
    HbmProfState &P = hbm_prof();
    std::lock_guard<std::mutex> g(P.mu);
    const bool on = mode != 0;
    if (mode == 1)
        for (int i = 0; i < HBM_SLOTS; ++i) {
            for (auto &r : P.recs[i]) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
            P.recs[i].clear(); P.bytes[i] = 0;
        }
    P.on = on;
}

hipError_t hbm_profile_read(int slot, double *ms_sum, int *launches, double *alg_bytes_sum)
{
    HbmProfState &P = hbm_prof();
    std::lock_guard<std::mutex> g(P.mu);
    if (slot < 0 || slot >= HBM_SLOTS) return hipErrorInvalidValue;
    double ms = 0;
    for (auto &r : P.recs[slot]) {
        float m = 0.f;
        const hipError_t e = hipEventElapsedTime(&m, r.a, r.b);      // the stream must have been synchronised
        if (e != hipSuccess) return e;
        ms += m;
    }
    *ms_sum = ms; *launches = (int)P.recs[slot].size(); *alg_bytes_sum = P.bytes[slot];
    return hipSuccess;
}

hipError_t hbm_profile_begin(int slot, double alg_bytes, hipEvent_t *a, hipEvent_t *b)
{
    HbmProfState &P = hbm_prof();
    *a = *b = nullptr;
    if (!P.on || slot < 0) return hipSuccess;        // slot < 0: a launch that is not timed
    HbmProfState::Rec r;
    hipError_t e = hipEventCreate(&r.a);
    if (e != hipSuccess) return e;
    e = hipEventCreate(&r.b);
    if (e != hipSuccess) { (void)hipEventDestroy(r.a); return e; }
    std::lock_guard<std::mutex> g(P.mu);
    P.recs[slot].push_back(r); P.bytes[slot] += alg_bytes;
    *a = r.a; *b = r.b;
    return hipSuccess;
}
}  // namespace vstab
