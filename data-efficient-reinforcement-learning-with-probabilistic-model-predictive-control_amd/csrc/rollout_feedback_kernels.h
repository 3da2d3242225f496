// rollout_feedback_kernels.h -- the per-candidate kernels of the closed-loop moment-matched rollout, shared by the forward
// (rollout_feedback.hip: gpmpc_rollout_feedback) and by the forward its gradient recomputes (rollout_feedback_backward.hip:
// gpmpc_rollout_feedback_backward), so that the recomputed trajectory and model inputs have the forward's bits.
//   write_model_input             the model input of a step from (mu_t, Sigma_t) in LDS: mean and G Sigma_t G^T
//   rollout_feedback_init_kernel  one wavefront per candidate: index 0 of the stored trajectory, the model input of step 0.
//   rollout_feedback_step_kernel  one wavefront per candidate, after the moment launches of step t: C, mu_{t+1}, Sigma_{t+1} into the
//                                 stored trajectory and the model input of step t + 1 from K_{t+1}.
#pragma once
#include "device_common.h"

namespace gpmpc_hip {

namespace {

struct FbArgs {
    const double* actions;   // (rows, H, A) of this chunk
    const double* gains;     // (H, A, D) of the chunk's first candidate
    long long gain_stride;   // doubles between two candidates' gains (0: one gain sequence shared by all)
    double* mu;              // (rows, H + 1, D) of this chunk
    double* Sig;             // (rows, H + 1, D, D) of this chunk
    double* xin;             // (rows, E) model input means of the step at hand
    double* sin;             // (rows, E, E) model input covariances
    const double* M;         // (rows, D) the step's moments ...
    const double* S;         // (rows, D, D)
    const double* V;         // (rows, E, D)
    int E, D, A, H, t, include_time;
    double time0;
    double mu0[kMaxD];       // read by the init kernel
    double S0[kMaxD * kMaxD];
};

// The model input of step t for candidate b from (s_mu, s_S) = (mu_t, Sigma_t) in LDS: mean [mu_t | ubar_t | time0 + t] and
// covariance G Sigma_t G^T, G = [I ; K_t ; 0].  Only the upper triangle of s_S is read, and every entry (i, j) is the expression
// of (min, max): exactly symmetric.  The callers have synchronised after writing s_mu / s_S.  Leaves K_t in s_K and K_t Sigma_t in
// s_KS.
__device__ inline void write_model_input(const FbArgs& p, int b, int t, const double (&s_mu)[kMaxD],
                                         const double (&s_S)[kMaxD][kMaxD], double (&s_K)[kMaxE][kMaxD],
                                         double (&s_KS)[kMaxE][kMaxD]) {
    const int tid = threadIdx.x;
    const int D = p.D, E = p.E, A = p.A, H = p.H;
    const double* K = p.gains + (size_t)b * (size_t)p.gain_stride + (size_t)t * A * D;       // [action][state]
    for (int idx = tid; idx < A * D; idx += 64) s_K[idx / D][idx % D] = K[idx];
    __syncthreads();
    for (int idx = tid; idx < A * D; idx += 64) {                // K Sigma_t, the states in order
        const int u = idx / D, j = idx - u * D;
        double v = 0.0;
        for (int k = 0; k < D; ++k) v = fma(s_K[u][k], k <= j ? s_S[k][j] : s_S[j][k], v);
        s_KS[u][j] = v;
    }
    __syncthreads();
    double* sg = p.sin + (size_t)b * E * E;
    for (int idx = tid; idx < E * E; idx += 64) {
        const int i = idx / E, j = idx - i * E;
        const int r = i < j ? i : j, c = i < j ? j : i;
        double v = 0.0;                                          // the time row and column
        if (c < D) v = s_S[r][c];
        else if (c < D + A && r < D) v = s_KS[c - D][r];
        else if (c < D + A) {                                    // (K Sigma_t) K^T, the states in order
            for (int k = 0; k < D; ++k) v = fma(s_KS[r - D][k], s_K[c - D][k], v);
        }
        sg[idx] = v;
    }
    double* xq = p.xin + (size_t)b * E;
    if (tid < D) xq[tid] = s_mu[tid];
    if (tid < A) xq[D + tid] = p.actions[((size_t)b * H + t) * A + tid];
    if (p.include_time && tid == 0) xq[E - 1] = p.time0 + (double)t;
}

// Index 0 of the stored trajectory (the caller's mu0 and S0 as they are) and the model input of step 0.
__global__ __launch_bounds__(64) void rollout_feedback_init_kernel(FbArgs p) {
    __shared__ double s_mu[kMaxD];
    __shared__ double s_S[kMaxD][kMaxD];
    __shared__ double s_K[kMaxE][kMaxD];
    __shared__ double s_KS[kMaxE][kMaxD];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int D = p.D, H = p.H;
    double* mu = p.mu + (size_t)b * (H + 1) * D;
    double* Sg = p.Sig + (size_t)b * (H + 1) * D * D;
    for (int idx = tid; idx < D * D; idx += 64) {
        Sg[idx] = p.S0[idx];
        s_S[idx / D][idx % D] = p.S0[idx];
    }
    if (tid < D) {
        mu[tid] = p.mu0[tid];
        s_mu[tid] = p.mu0[tid];
    }
    __syncthreads();
    write_model_input(p, b, 0, s_mu, s_S, s_K, s_KS);
}

// One wavefront per candidate, after the moment launches of step t: with the step's input covariance Sigma_in (its state block is
// Sigma_t) and moments M, S, V
//   C = Sigma_in[:D, :] V (the inputs in order, the zero time column left out),  mu' = mu_t + M,
//   Sigma' = (Sigma_t + S) + (C + C^T) for a <= b, mirrored
// into index t + 1 of the stored trajectory, and the model input of step t + 1 where there is one.
__global__ __launch_bounds__(64) void rollout_feedback_step_kernel(FbArgs p) {
    __shared__ double s_in[kMaxD][kMaxE];            // the first D rows of Sigma_in
    __shared__ double s_V[kMaxE][kMaxD];             // V [input][output]
    __shared__ double s_C[kMaxD][kMaxD];
    __shared__ double s_mu[kMaxD];
    __shared__ double s_S[kMaxD][kMaxD];             // Sigma_{t+1}
    __shared__ double s_K[kMaxE][kMaxD];
    __shared__ double s_KS[kMaxE][kMaxD];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int D = p.D, E = p.E, A = p.A, H = p.H, t = p.t, DA = D + A;
    const double* sg = p.sin + (size_t)b * E * E;
    const double* Vm = p.V + (size_t)b * E * D;
    const double* Sm = p.S + (size_t)b * D * D;
    double* mu_n = p.mu + ((size_t)b * (H + 1) + t + 1) * D;
    double* Sg_n = p.Sig + ((size_t)b * (H + 1) + t + 1) * D * D;
    for (int idx = tid; idx < D * E; idx += 64) s_in[idx / E][idx % E] = sg[idx];
    for (int idx = tid; idx < E * D; idx += 64) s_V[idx / D][idx % D] = Vm[idx];
    if (tid < D) {
        const double v = p.xin[(size_t)b * E + tid] + p.M[(size_t)b * D + tid];
        mu_n[tid] = v;
        s_mu[tid] = v;
    }
    __syncthreads();
    for (int idx = tid; idx < D * D; idx += 64) {
        const int a = idx / D, c = idx - a * D;
        double v = 0.0;
        for (int e = 0; e < DA; ++e) v = fma(s_in[a][e], s_V[e][c], v);
        s_C[a][c] = v;
    }
    __syncthreads();
    for (int idx = tid; idx < D * D; idx += 64) {                // a <= c, mirrored: exactly symmetric
        const int a = idx / D, c = idx - a * D;
        if (a > c) continue;
        const double v = (s_in[a][c] + Sm[a * D + c]) + (s_C[a][c] + s_C[c][a]);
        s_S[a][c] = v;
        s_S[c][a] = v;
        Sg_n[a * D + c] = v;
        Sg_n[c * D + a] = v;
    }
    if (t + 1 >= H) return;
    __syncthreads();
    write_model_input(p, b, t + 1, s_mu, s_S, s_K, s_KS);
}

}  // namespace

}  // namespace gpmpc_hip
