// lqr_gains_plan.h -- host-side planning of gpmpc_lqr_gains (lqr_gains.hip): how many candidates a chunk holds and where each
// array of its workspace starts.  Plain C++ (no HIP), so that a stand-alone host program can run it under a sanitizer
// (tools/host_checks/lqr_gains_plan_check.cpp).
#pragma once
#include <cstddef>

namespace gpmpc_hip {

constexpr int kLqrMaxA = 8;                                // action dimensions of the Riccati kernel (its LDS arrays and solves)
constexpr int kLqrRound = 64;                              // an automatic chunk is a multiple of the tile height of the tile kernel
constexpr size_t kLqrWsBudget = (size_t)16 << 20;          // bytes of workspace per chunk (or one 64-candidate chunk's need if that is more)

struct LqrGainsPlan {
    long long chunk;         // candidates per chunk (>= 1)
    // offsets (doubles) of the arrays of one chunk, in this order, and their sizes
    size_t xq, n_xq;         // (chunk, E) model inputs [mu_t | ubar_t | time0 + t] of the step at hand
    size_t M, n_M;           // (chunk, D) the step's posterior mean
    size_t V, n_V;           // (H, chunk, E, D) every step's mean Jacobian (the Riccati kernel reads its D + A state / action rows)
    size_t total;            // doubles
};

// count: candidates; opt_chunk: option "lqr_gains_chunk_points" (0 = auto).  Needs D, E, H >= 1 and count >= 1.
inline void plan_lqr_gains(int D, int E, int H, long long count, long long opt_chunk, LqrGainsPlan& p) {
    const size_t per_row = (size_t)E + (size_t)D + (size_t)H * E * D;
    long long chunk = (long long)(kLqrWsBudget / (sizeof(double) * per_row)) / kLqrRound * kLqrRound;
    if (opt_chunk > 0) chunk = opt_chunk;
    if (chunk < 1) chunk = kLqrRound;
    if (chunk > count) chunk = count;
    p.chunk = chunk;
    const size_t c = (size_t)chunk;
    size_t o = 0;
    auto take = [&](size_t& off, size_t& n, size_t size) { off = o; n = size; o += size; };
    take(p.xq, p.n_xq, c * E);
    take(p.M, p.n_M, c * D);
    take(p.V, p.n_V, (size_t)H * c * E * D);
    p.total = o;
}

}  // namespace gpmpc_hip
