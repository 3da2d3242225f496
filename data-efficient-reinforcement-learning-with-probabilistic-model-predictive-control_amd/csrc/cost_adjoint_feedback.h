// cost_adjoint_feedback.h -- the closed-loop stage-cost adjoint on one wavefront, shared by the two closed-loop gradients:
// gpmpc_rollout_linear_feedback_backward (moments_linear_backward.hip) and gpmpc_rollout_feedback_backward
// (rollout_feedback_backward.hip).  The open-loop and terminal form, cost_adjoint_wave, and the seeded weights are grad_kernels.h's.
#pragma once
#include "grad_kernels.h"

namespace gpmpc_hip {

namespace {

// Closed-loop form of cost_adjoint_wave for a stage t < H: the quadratic cost sees Sigma_z = G Sigma_t G^T with G = [I ; K]
// (K (A, D) row-major), so besides (mu, Sigma, u) there is a partial wrt K.  With Q = W Sigma_z W (W not assumed symmetric):
//   Sz_bar = wm W^T + 4 wv (Q^T + (W^T e)(W e)^T),   e_bar = wm (W + W^T) e + 4 wv (Q + Q^T) e
//   gSig = G^T Sz_bar G,   gK = action rows of (Sz_bar + Sz_bar^T) G Sigma_t,   gmu = e_bar[:D],   gu = e_bar[D:]
// and the constraint term of cost_adjoint_wave (state marginals only: no partial wrt K).  One wavefront; `tmp` is its scratch,
// cost_adjoint_feedback_tmp(D, A) doubles.
__host__ __device__ constexpr int cost_adjoint_feedback_tmp(int D, int A) { return (D + A) * D + 3 * (D + A) * (D + A) + 3 * (D + A); }

__device__ inline void cost_adjoint_feedback_wave(int lane, int D, int A, const double* mu, const double* Sg, const double* act,
                                                  const double* K, const double* target, const double* Wm, const double* smin,
                                                  const double* smax, bool use_constraints, double wm, double wv, double* tmp,
                                                  double* gmu, double* gSig, double* gu, double* gK) {
    const int n = D + A;
    double* GS = tmp;            // G Sigma_t  (n x D)
    double* Sz = GS + n * D;     // Sigma_z  (n x n); then Sz_bar
    double* WS = Sz + n * n;     // W Sigma_z  (n x n); then Sz_bar G  (n x D)
    double* Q = WS + n * n;      // W Sigma_z W
    double* err = Q + n * n;
    double* We = err + n;
    double* WTe = We + n;
    for (int i = lane; i < n; i += 64) err[i] = (i < D ? mu[i] : act[i - D]) - target[i];
    for (int idx = lane; idx < n * D; idx += 64) {
        const int i = idx / D, j = idx - i * D;
        double v;
        if (i < D) {
            v = Sg[i * D + j];
        } else {
            v = 0.0;
            for (int k = 0; k < D; ++k) v = fma(K[(i - D) * D + k], Sg[k * D + j], v);
        }
        GS[idx] = v;
    }
    wave_lds_sync();
    for (int idx = lane; idx < n * n; idx += 64) {               // Sigma_z = (G Sigma_t) G^T
        const int i = idx / n, j = idx - i * n;
        double v;
        if (j < D) {
            v = GS[i * D + j];
        } else {
            v = 0.0;
            for (int k = 0; k < D; ++k) v = fma(GS[i * D + k], K[(j - D) * D + k], v);
        }
        Sz[idx] = v;
    }
    for (int i = lane; i < n; i += 64) {
        double a = 0.0, b = 0.0;
        for (int k = 0; k < n; ++k) { a = fma(Wm[i * n + k], err[k], a); b = fma(Wm[k * n + i], err[k], b); }
        We[i] = a; WTe[i] = b;
    }
    wave_lds_sync();
    for (int idx = lane; idx < n * n; idx += 64) {
        const int i = idx / n, j = idx - i * n;
        double v = 0.0;
        for (int k = 0; k < n; ++k) v = fma(Wm[i * n + k], Sz[k * n + j], v);
        WS[idx] = v;
    }
    wave_lds_sync();
    for (int idx = lane; idx < n * n; idx += 64) {
        const int i = idx / n, j = idx - i * n;
        double v = 0.0;
        for (int k = 0; k < n; ++k) v = fma(WS[i * n + k], Wm[k * n + j], v);
        Q[idx] = v;
    }
    wave_lds_sync();
    for (int idx = lane; idx < n * n; idx += 64) {               // Sz_bar (over Sigma_z)
        const int i = idx / n, j = idx - i * n;
        Sz[idx] = wm * Wm[j * n + i] + wv * 4.0 * (Q[j * n + i] + WTe[i] * We[j]);
    }
    for (int i = lane; i < n; i += 64) {
        double v = 0.0;
        for (int k = 0; k < n; ++k) v = fma(Q[i * n + k] + Q[k * n + i], err[k], v);
        v = wm * (We[i] + WTe[i]) + wv * 4.0 * v;
        if (i < D) {
            if (use_constraints) {
                const double sq = Sg[i * D + i];
                const double zmin = (smin[i] - mu[i]) / sq, zmax = (smax[i] - mu[i]) / sq;
                v += wm * (-exp(-0.5 * zmin * zmin) + exp(-0.5 * zmax * zmax)) * 0.3989422804014327 / sq;
            }
            gmu[i] = v;
        } else {
            gu[i - D] = v;
        }
    }
    wave_lds_sync();
    double* SG = WS;                                             // Sz_bar G  (n x D, over W Sigma_z)
    for (int idx = lane; idx < n * D; idx += 64) {
        const int i = idx / D, j = idx - i * D;
        double v = 0.0;
        for (int u = 0; u < A; ++u) v = fma(Sz[i * n + D + u], K[u * D + j], v);
        SG[idx] = Sz[i * n + j] + v;
    }
    for (int idx = lane; idx < A * D; idx += 64) {               // action rows of (Sz_bar + Sz_bar^T) (G Sigma_t)
        const int u = idx / D, j = idx - u * D;
        double v = 0.0;
        for (int k = 0; k < n; ++k) v = fma(Sz[(D + u) * n + k] + Sz[k * n + D + u], GS[k * D + j], v);
        gK[idx] = v;
    }
    wave_lds_sync();
    for (int idx = lane; idx < D * D; idx += 64) {               // G^T (Sz_bar G)
        const int i = idx / D, j = idx - i * D;
        double v = 0.0;
        for (int u = 0; u < A; ++u) v = fma(K[u * D + i], SG[(D + u) * D + j], v);
        v = SG[i * D + j] + v;
        if (use_constraints && i == j) {
            const double sq = Sg[i * D + i];                     // the variance as sigma, as cost_adjoint_wave
            const double zmin = (smin[i] - mu[i]) / sq, zmax = (smax[i] - mu[i]) / sq;
            const double pmin = exp(-0.5 * zmin * zmin) * 0.3989422804014327, pmax = exp(-0.5 * zmax * zmax) * 0.3989422804014327;
            v += wm * (-pmin * zmin + pmax * zmax) / sq;
        }
        gSig[idx] = v;
    }
}

}  // namespace

}  // namespace gpmpc_hip
