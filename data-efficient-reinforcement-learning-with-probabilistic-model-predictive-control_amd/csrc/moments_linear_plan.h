// moments_linear_plan.h -- host-side planning of gpmpc_moments_linear / gpmpc_rollout_linear (moments_linear.hip): how many points
// or candidates a chunk holds and how large its workspace is.  Plain C++ (no HIP), so that a stand-alone host program can run it
// under a sanitizer (tools/host_checks/moments_linear_plan_check.cpp).
#pragma once
#include <cstddef>

namespace gpmpc_hip {

constexpr int kLinBM = 64;                              // query rows per workgroup of the tile kernel
constexpr int kLinBN = 256;                             // columns of iK per workgroup
constexpr size_t kLinWsBudget = (size_t)16 << 20;       // bytes of workspace per chunk (or one 64-row tile's need if that is more)

struct LinearPlan {
    int nCB;                 // column blocks of iK
    int NW;                  // partial sums per (output, column block, row): sum P k | sum k beta | E sums beta k (x_j - m)
    long long chunk;         // points / candidates per chunk (>= 1)
    long long Mc;            // row stride of the workspace arrays: chunk rounded up to the tile height
    size_t part;             // doubles: partial sums (D, nCB, NW, Mc)
    size_t xq;               // doubles: model inputs of the chunk (Mc, E) (rollout only)
    size_t traj;             // doubles: the chunk's trajectory (chunk, H + 1, D + D D) where the caller keeps none (rollout only)
    size_t total;            // doubles
};

// count: points (H = 0: gpmpc_moments_linear) or candidates (H >= 1: gpmpc_rollout_linear, own_traj: the caller gave no mu / Sig
// outputs); opt_chunk: option "moments_linear_chunk_points" (0 = auto).  Needs N, D, E >= 1 and count >= 1.
inline void plan_moments_linear(int N, int D, int E, long long count, int H, bool own_traj, long long opt_chunk, LinearPlan& p) {
    p.nCB = (N + kLinBN - 1) / kLinBN;
    p.NW = E + 2;
    size_t per_row = (size_t)D * p.nCB * p.NW;
    if (H > 0) per_row += (size_t)E;
    const size_t per_traj = (H > 0 && own_traj) ? (size_t)(H + 1) * ((size_t)D + (size_t)D * D) : 0;
    per_row += per_traj;
    long long chunk = (long long)(kLinWsBudget / (sizeof(double) * per_row)) / kLinBM * kLinBM;
    if (opt_chunk > 0) chunk = opt_chunk;
    if (chunk < 1) chunk = kLinBM;
    if (chunk > count) chunk = count;
    p.chunk = chunk;
    p.Mc = (chunk + kLinBM - 1) / kLinBM * kLinBM;
    p.part = (size_t)D * p.nCB * p.NW * (size_t)p.Mc;
    p.xq = H > 0 ? (size_t)p.Mc * E : 0;
    p.traj = per_traj * (size_t)chunk;
    p.total = p.part + p.xq + p.traj;
}

}  // namespace gpmpc_hip
