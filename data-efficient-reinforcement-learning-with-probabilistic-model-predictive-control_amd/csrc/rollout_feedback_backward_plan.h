// rollout_feedback_backward_plan.h -- host-side planning of gpmpc_rollout_feedback_backward (rollout_feedback_backward.hip): how
// many candidates a chunk holds and where the chunk's arrays lie in the entry's own workspace (Handle::fbbws).  Plain C++ (no HIP),
// so that a stand-alone host program can run it under a sanitizer (tools/host_checks/rollout_feedback_backward_plan_check.cpp).
// The workspaces of the moment kernels the entry launches every step (Handle::momws, Handle::mombws) are planned by run_moments
// and run_moments_backward themselves, not here.
#pragma once
#include <cstddef>

namespace gpmpc_hip {

constexpr size_t kFbbWsBudget = (size_t)16 << 20;       // bytes of workspace per chunk (or one candidate's need if that is more)
constexpr int kFbbRound = 8;                            // an automatic chunk is a multiple of the pair pass's points per workgroup

struct FeedbackBwdPlan {
    long long chunk;         // candidates per chunk (>= 1)
    // offsets in doubles from the start of the workspace, in this order; each array is (chunk, ...) unless said otherwise
    size_t xin;              // (chunk, E)       model input means of the step at hand (forward and reverse)
    size_t sin;              // (chunk, E, E)    model input covariances G Sigma_t G^T
    size_t M;                // (chunk, D)       the forward step's M and S (V goes to keepV)
    size_t S;                // (chunk, D, D)
    size_t mu;               // (chunk, H + 1, D)      the recomputed trajectory ...
    size_t Sig;              // (chunk, H + 1, D, D)
    size_t keepV;            // (H, chunk, E, D) STEP-major: every step's V, written by the moment kernels themselves
    size_t cv;               // (chunk, H + 1)   closed-loop cost variances (read with an objective seed only)
    size_t adj;              // (chunk, D + D D) lambda | Lambda between two reverse launches
    size_t Mb;               // (chunk, D)       the cotangents handed to the moment gradient: M_bar ...
    size_t Sb;               // (chunk, D, D)    S_bar
    size_t Vb;               // (chunk, E, D)    V_bar
    size_t xb;               // (chunk, E)       ... and what it returns: x_bar
    size_t Pb;               // (chunk, E, E)    P, the symmetric part
    size_t zero_gains;       // (H, A, D) zeros: the shared gain sequence of a call without gains (no_gains)
    size_t total;            // doubles
};

// doubles one candidate needs (everything but the zero gains)
inline size_t feedback_bwd_per_candidate(int D, int E, int H) {
    const size_t d = (size_t)D, e = (size_t)E, t1 = (size_t)H + 1;
    return (e + e * e + d + d * d) + t1 * (d + d * d) + (size_t)H * e * d + t1 + (d + d * d) + (d + d * d + e * d) + (e + e * e);
}

// B candidates, horizon H; no_gains: gains == NULL; opt_chunk: option "rollout_feedback_backward_chunk_points" (0 = auto).
// Needs D, E, B, H >= 1, A >= 0.
inline void plan_rollout_feedback_backward(int D, int E, int A, long long B, int H, bool no_gains, long long opt_chunk,
                                           FeedbackBwdPlan& p) {
    const size_t per_cand = feedback_bwd_per_candidate(D, E, H);
    long long chunk = (long long)(kFbbWsBudget / (sizeof(double) * per_cand));
    if (chunk >= kFbbRound) chunk = chunk / kFbbRound * kFbbRound;
    if (opt_chunk > 0) chunk = opt_chunk;
    if (chunk < 1) chunk = 1;
    if (chunk > B) chunk = B;
    p.chunk = chunk;
    const size_t c = (size_t)chunk, d = (size_t)D, e = (size_t)E, t1 = (size_t)H + 1;
    p.xin = 0;
    p.sin = p.xin + c * e;
    p.M = p.sin + c * e * e;
    p.S = p.M + c * d;
    p.mu = p.S + c * d * d;
    p.Sig = p.mu + c * t1 * d;
    p.keepV = p.Sig + c * t1 * d * d;
    p.cv = p.keepV + (size_t)H * c * e * d;
    p.adj = p.cv + c * t1;
    p.Mb = p.adj + c * (d + d * d);
    p.Sb = p.Mb + c * d;
    p.Vb = p.Sb + c * d * d;
    p.xb = p.Vb + c * e * d;
    p.Pb = p.xb + c * e;
    p.zero_gains = p.Pb + c * e * e;
    p.total = p.zero_gains + (no_gains ? (size_t)H * A * D : 0);
}

}  // namespace gpmpc_hip
