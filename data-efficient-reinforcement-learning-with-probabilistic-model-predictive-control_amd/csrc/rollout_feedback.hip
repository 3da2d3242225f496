// rollout_feedback.hip -- the moment-matched horizon rollout in closed loop (gpmpc_rollout_feedback): the policy is
// u = ubar_t + K_t (x - mu_t), x ~ N(mu_t, Sigma_t).  Per step t, with G_t = [I_D ; K_t ; 0] (E x D, the time row zero):
//   input mean [mu_t | ubar_t | time0 + t],  input covariance Sigma_in = G_t Sigma_t G_t^T (blocks Sigma_t, K_t Sigma_t, its
//   transpose, K_t Sigma_t K_t^T; formed for i <= j and mirrored, the time row and column exactly zero)
//   M, S, V = the moments of gpmpc_moments at that input (moments.hip: run_moments, its kernels unchanged)
//   C = (first D rows of Sigma_in) V = Sigma_t (V_s + K_t^T V_u)
//   mu_{t+1} = mu_t + M,  Sigma_{t+1} = Sigma_t + S + C + C^T  (for a <= b, mirrored)
// This is predict_trajectory's recurrence (gp_model.py:60-110) fed the policy's full input covariance.  Sigma_in has rank D in E
// dimensions; the moment kernels only ever factorise I + Lambda^1/2 Sigma_in Lambda^1/2, never Sigma_in itself.
//
// Structure ("Closed-loop moment-matched rollouts"): batch-major, per chunk of candidates; the per-candidate kernels are
// in rollout_feedback_kernels.h, shared with the forward that gpmpc_rollout_feedback_backward recomputes
//   rollout_feedback_init_kernel  one wavefront per candidate: index 0 of the stored trajectory, the model input of step 0.
//   run_moments                   per horizon step, on the chunk's inputs: setup, point, pair and finish launches.
//   rollout_feedback_step_kernel  one wavefront per candidate, after them: C, mu_{t+1}, Sigma_{t+1} into the stored trajectory and
//                                 the model input of step t + 1 from K_{t+1}.
//   traj_cost_feedback_kernel     (moments_linear.hip) the closed-loop stage costs and objective of the stored trajectory.
// A call without gains runs the same kernels on a zeroed shared gain sequence in the workspace.  Every sum runs in an order fixed
// by D, A and E alone, the moment kernels' by N, E and the pair: a candidate's bits do not depend on the batch, on its place in it,
// on either chunk option or on the gain layout.  Plain kernels: no atomics, no waits between workgroups.  The workspace
// (Handle::fbws) is this file's own, laid out by plan_rollout_feedback (rollout_feedback_plan.h); run_moments uses Handle::momws.
#include "rollout_feedback_kernels.h"
#include "rollout_feedback_plan.h"

namespace gpmpc_hip {

// a: filled by the entry point (model, cost settings, actions, shape, initial state, outputs -- each output may be NULL).
// gains (B, H, A, D) when per_candidate, else (H, A, D) shared by all candidates, or NULL: the all-zero shared sequence.
int run_rollout_feedback(Handle* h, const RolloutArgs& a, hipStream_t s, const double* gains, bool per_candidate) {
    const int D = a.D, E = a.E, A = a.A, H = a.H, B = a.B;
    const bool own_traj = !a.mu_out || !a.Sig_out;
    const bool costs = a.cm_out || a.cv_out || a.J_out;
    FeedbackPlan pl;
    plan_rollout_feedback(D, E, A, B, H, own_traj, gains == nullptr, h->opt_rollout_feedback_chunk, pl);
    int rc = grow(h, h->fbws, pl.total);
    if (rc) return rc;
    double* ws = h->fbws.p;
    if (!gains) {
        if (pl.total > pl.zero_gains)
            GPMPC_HIP_CHECK(h, hipMemsetAsync(ws + pl.zero_gains, 0, (pl.total - pl.zero_gains) * sizeof(double), s));
        gains = ws + pl.zero_gains;
        per_candidate = false;
    }
    FbArgs q{};
    q.xin = ws + pl.xin; q.sin = ws + pl.sin;
    q.M = ws + pl.M; q.S = ws + pl.S; q.V = ws + pl.V;
    q.E = E; q.D = D; q.A = A; q.H = H;
    q.include_time = a.include_time; q.time0 = a.time0;
    for (int d = 0; d < D; ++d) q.mu0[d] = a.mu0[d];
    for (int d = 0; d < D * D; ++d) q.S0[d] = a.S0[d];
    q.gain_stride = per_candidate ? (long long)H * A * D : 0;
    for (long long b0 = 0; b0 < B; b0 += pl.chunk) {
        const int rows = (int)((B - b0) < pl.chunk ? (B - b0) : pl.chunk);
        q.actions = a.actions + (size_t)b0 * H * A;
        q.gains = gains + (size_t)b0 * (size_t)q.gain_stride;
        q.mu = a.mu_out ? a.mu_out + (size_t)b0 * (H + 1) * D : ws + pl.traj_mu;
        q.Sig = a.Sig_out ? a.Sig_out + (size_t)b0 * (H + 1) * D * D : ws + pl.traj_Sig;
        q.t = 0;
        hipLaunchKernelGGL(rollout_feedback_init_kernel, dim3(rows), dim3(64), 0, s, q);
        for (int t = 0; t < H; ++t) {
            rc = run_moments(h, q.xin, q.sin, rows, ws + pl.M, ws + pl.S, ws + pl.V, s);
            if (rc) return rc;
            q.t = t;
            hipLaunchKernelGGL(rollout_feedback_step_kernel, dim3(rows), dim3(64), 0, s, q);
        }
        GPMPC_HIP_CHECK(h, hipGetLastError());
        if (costs) {                                  // closed-loop stage costs + objective of the chunk's stored trajectory
            double* cm = a.cm_out ? a.cm_out + (size_t)b0 * (H + 1) : nullptr;
            double* cv = a.cv_out ? a.cv_out + (size_t)b0 * (H + 1) : nullptr;
            double* J = a.J_out ? a.J_out + b0 : nullptr;
            rc = launch_traj_cost_feedback(h, a, rows, q.mu, q.Sig, q.actions, q.gains, q.gain_stride, cm, cv, J, s);
            if (rc) return rc;
        }
    }
    return GPMPC_OK;
}

}  // namespace gpmpc_hip
