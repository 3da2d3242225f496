// rollout_feedback_plan.h -- host-side planning of gpmpc_rollout_feedback (rollout_feedback.hip): how many candidates a chunk holds
// and where the chunk's arrays lie in the entry's own workspace (Handle::fbws).  Plain C++ (no HIP), so that a stand-alone host
// program can run it under a sanitizer (tools/host_checks/rollout_feedback_plan_check.cpp).  The workspace of the moment kernels
// the entry launches every horizon step (Handle::momws) is planned by run_moments itself, not here.
#pragma once
#include <cstddef>

namespace gpmpc_hip {

constexpr size_t kFbWsBudget = (size_t)16 << 20;        // bytes of workspace per chunk (or one candidate's need if that is more)
constexpr int kFbRound = 8;                             // an automatic chunk is a multiple of the pair pass's points per workgroup

struct FeedbackPlan {
    long long chunk;         // candidates per chunk (>= 1)
    // offsets in doubles from the start of the workspace, in this order; each array is (chunk, ...)
    size_t xin;              // (chunk, E)       model input means of the step at hand
    size_t sin;              // (chunk, E, E)    model input covariances G Sigma_t G^T
    size_t M;                // (chunk, D)       the step's moments ...
    size_t S;                // (chunk, D, D)
    size_t V;                // (chunk, E, D)
    size_t traj_mu;          // (chunk, H + 1, D)      the chunk's trajectory where the caller keeps none (own_traj) ...
    size_t traj_Sig;         // (chunk, H + 1, D, D)
    size_t zero_gains;       // (H, A, D) zeros: the shared gain sequence of a call without gains (no_gains)
    size_t total;            // doubles
};

// B candidates, horizon H; own_traj: the caller gave no mu / Sig outputs; no_gains: gains == NULL; opt_chunk: option
// "rollout_feedback_chunk_points" (0 = auto).  Needs D, E, B, H >= 1, A >= 0.
inline void plan_rollout_feedback(int D, int E, int A, long long B, int H, bool own_traj, bool no_gains, long long opt_chunk,
                                  FeedbackPlan& p) {
    const size_t step = (size_t)E + (size_t)E * E + (size_t)D + (size_t)D * D + (size_t)E * D;
    const size_t traj_mu = own_traj ? (size_t)(H + 1) * D : 0;
    const size_t traj_Sig = own_traj ? (size_t)(H + 1) * D * D : 0;
    const size_t per_cand = step + traj_mu + traj_Sig;
    long long chunk = (long long)(kFbWsBudget / (sizeof(double) * per_cand));
    if (chunk >= kFbRound) chunk = chunk / kFbRound * kFbRound;
    if (opt_chunk > 0) chunk = opt_chunk;
    if (chunk < 1) chunk = 1;
    if (chunk > B) chunk = B;
    p.chunk = chunk;
    const size_t c = (size_t)chunk;
    p.xin = 0;
    p.sin = p.xin + c * E;
    p.M = p.sin + c * E * E;
    p.S = p.M + c * D;
    p.V = p.S + c * D * D;
    p.traj_mu = p.V + c * E * D;
    p.traj_Sig = p.traj_mu + c * traj_mu;
    p.zero_gains = p.traj_Sig + c * traj_Sig;
    p.total = p.zero_gains + (no_gains ? (size_t)H * A * D : 0);
}

}  // namespace gpmpc_hip
