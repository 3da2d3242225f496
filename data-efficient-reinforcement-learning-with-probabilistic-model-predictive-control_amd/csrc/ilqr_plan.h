// ilqr_plan.h -- host-side planning of gpmpc_ilqr_* (ilqr.hip): how many candidates a chunk holds and where each array of its
// workspace (Handle::ilqrws) starts.  Plain C++ (no HIP), so that a stand-alone host program can run it under a sanitizer
// (tools/host_checks/ilqr_plan_check.cpp).
#pragma once
#include <cstddef>

namespace gpmpc_hip {

constexpr int kIlqrRound = 64;                              // an automatic chunk is a multiple of the tile height of the tile kernel
constexpr size_t kIlqrWsBudget = (size_t)16 << 20;          // bytes of workspace per chunk (or one chunk's need if that is more)

struct IlqrPlan {
    long long chunk;         // candidates per chunk (>= 1); the forward pass runs chunk * L rows
    // offsets (doubles) of the arrays of one chunk, in this order, and their sizes
    size_t xq, n_xq;         // (chunk * L, E) model inputs of the step at hand (the backward pass uses the first chunk rows)
    size_t M, n_M;           // (chunk * L, D) the step's posterior mean
    size_t V, n_V;           // (H, chunk, E, D) every step's mean Jacobian of the nominal trajectory
    size_t tmu, n_tmu;       // (chunk * L, H + 1, D) the trial trajectories, when the caller does not take them
    size_t total;            // doubles
};

// count: candidates; L: line-search steps; opt_chunk: option "ilqr_chunk_points" (0 = auto).  Needs D, E, H, L >= 1 and count >= 1.
inline void plan_ilqr(int D, int E, int H, int L, long long count, long long opt_chunk, IlqrPlan& p) {
    const size_t per_row = (size_t)L * E + (size_t)L * D + (size_t)H * E * D + (size_t)L * (H + 1) * D;
    long long chunk = (long long)(kIlqrWsBudget / (sizeof(double) * per_row)) / kIlqrRound * kIlqrRound;
    if (opt_chunk > 0) chunk = opt_chunk;
    if (chunk < 1) chunk = kIlqrRound;
    if (chunk > count) chunk = count;
    p.chunk = chunk;
    const size_t c = (size_t)chunk;
    size_t o = 0;
    auto take = [&](size_t& off, size_t& n, size_t size) { off = o; n = size; o += size; };
    take(p.xq, p.n_xq, c * L * E);
    take(p.M, p.n_M, c * L * D);
    take(p.V, p.n_V, (size_t)H * c * E * D);
    take(p.tmu, p.n_tmu, c * L * (size_t)(H + 1) * D);
    p.total = o;
}

}  // namespace gpmpc_hip
