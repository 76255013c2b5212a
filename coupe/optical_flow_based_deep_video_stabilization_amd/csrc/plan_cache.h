// Per-geometry plans that live for the process (train_conv_api.cpp): the cache and the upload of a plan's index table, each stated once.
#pragma once
#include <array>
#include <cstdint>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

#include <hip/hip_runtime.h>

// Plans keyed by N ints of geometry.  on_device: the plan owns memory of the CURRENT device, which then is part of the key.
template <class Plan, size_t N> class PlanCache {
public:
    explicit PlanCache(bool on_device) : on_device_(on_device) {}

    // The plan of `geom`: the stored one, or what build(plan) fills into a zero-initialised plan, stored when build returns true (a
    // failed build is not stored and is tried again by the next call).  build runs under the cache's mutex: whatever it puts into the
    // plan is complete before any other thread can be handed it.
    template <class Build> bool get(const std::array<int, N> &geom, Plan &out, Build build)
    {
        int dev = 0;
        if (on_device_ && hipGetDevice(&dev) != hipSuccess) return false;
        const auto key = std::make_pair(dev, geom);
        std::lock_guard<std::mutex> lock(mu_);
        auto it = plans_.find(key);
        if (it == plans_.end()) {
            Plan d{};
            if (!build(d)) return false;
            it = plans_.emplace(key, d).first;
        }
        out = it->second;
        return true;
    }

private:
    const bool on_device_;
    std::mutex mu_;
    std::map<std::pair<int, std::array<int, N>>, Plan> plans_;
};

// A host-built index table in the current device's memory, or NULL.  Owned by the cache that stores the plan and never freed: a plan
// lives as long as the process.
inline int32_t *upload_table(const std::vector<int32_t> &tbl)
{
    int32_t *d = nullptr;
    if (hipMalloc(reinterpret_cast<void **>(&d), tbl.size() * sizeof(int32_t)) != hipSuccess) return nullptr;
    if (hipMemcpy(d, tbl.data(), tbl.size() * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(d); return nullptr; }
    return d;
}
