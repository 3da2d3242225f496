// lqr_gains.hip -- the LQR feedback gains of the linearisation along every candidate's nominal trajectory (gpmpc_lqr_gains): the
// gains K_t that gpmpc_rollout_linear_feedback takes as given.  Per candidate and step t the model input is
// [mu_t | ubar_t | time0 + t], mu_0 = mu0, mu_{t+1} = mu_t + M, with M and the mean Jacobian V (E x D) of gpmpc_moments_linear at
// that input; no covariance enters and no K* iK product runs.  With V_s / V_u the state / action rows of V,
//   A_t = I + V_s^T (D x D),   B_t = V_u^T (D x A)
// and, on the symmetric part W_s of the loaded stage weight (Q | N ; N^T | R) and P_H = sym(W_T), for t = H-1 .. 0
//   F = P_{t+1} A_t,  Huu = R + B_t^T P_{t+1} B_t + reg I,  Hux = N^T + B_t^T F,  K_t = -Huu^-1 Hux,  P_t = Q + A_t^T F + Hux^T K_t.
//
// Structure ("LQR gains"; the two kernels live in lqr_riccati_kernel.h, which the iLQR's backward sweep shares):
//   lqr_inputs_kernel     one thread per (candidate, model input): the model inputs of step t (t = 0: from mu0; else mu += M).
//   run_moments_linear    per step, on the chunk's model inputs, S NULL: its no-matrix-product form; the existing tile and finish
//                         kernels, unchanged.  M goes to the chunk's M array, V to slot t of the chunk's V array.
//   lqr_riccati_kernel    after the H steps: one wavefront per candidate, lanes over matrix elements, every matrix in LDS with an
//                         odd row pitch; the A x A Cholesky factorisation runs on the wavefront (A <= 8 dependent pivots), the two
//                         triangular solves one column of Hux per lane.  The next step's V rides in registers under the algebra.
// Every sum runs in an order fixed by N, E, D and A alone: a candidate's gains, cost-to-go and flag do not depend on the batch, on
// its place in it or on the chunks.  Plain kernels: no atomics, no waits between workgroups.  The workspace (Handle::lqrws) is this
// file's own, sized by plan_lqr_gains (lqr_gains_plan.h); run_moments_linear keeps using its own (Handle::linws).
#include "lqr_riccati_kernel.h"

namespace gpmpc_hip {

int run_lqr_gains(Handle* h, const double* actions, const double* mu0_host, int B, int H, int A, int include_time, double time0,
                  double reg, double* gains_out, double* P_out, int* flags_out, hipStream_t s) {
    const int D = h->D, E = h->E;
    LqrGainsPlan pl;
    plan_lqr_gains(D, E, H, B, h->opt_lqr_gains_chunk, pl);
    int rc = grow(h, h->lqrws, pl.total);
    if (rc) return rc;
    double* ws = h->lqrws.p;
    LqrInputArgs in{};
    in.Xq = ws + pl.xq; in.M = ws + pl.M;
    in.E = E; in.D = D; in.A = A; in.H = H; in.include_time = include_time; in.time0 = time0;
    for (int d = 0; d < D; ++d) in.mu0[d] = mu0_host[d];
    LqrRiccatiArgs r{};
    r.V = ws + pl.V; r.cost = h->cost.p;
    r.E = E; r.D = D; r.A = A; r.H = H; r.reg = reg;
    for (long long b0 = 0; b0 < B; b0 += pl.chunk) {
        const int rows = (int)((B - b0) < pl.chunk ? (B - b0) : pl.chunk);
        in.rows = rows;
        in.actions = actions + (size_t)b0 * H * A;
        const unsigned blocks = (unsigned)(((long long)rows * E + 255) / 256);
        for (int t = 0; t < H; ++t) {
            in.t = t;
            hipLaunchKernelGGL(lqr_inputs_kernel, dim3(blocks), dim3(256), 0, s, in);
            rc = run_moments_linear(h, ws + pl.xq, nullptr, rows, ws + pl.M, nullptr, ws + pl.V + (size_t)t * rows * E * D, s);
            if (rc) return rc;
        }
        r.rows = rows;
        r.gains = gains_out + (size_t)b0 * H * A * D;
        r.P = P_out ? P_out + (size_t)b0 * (H + 1) * D * D : nullptr;
        r.flags = flags_out ? flags_out + b0 : nullptr;
        hipLaunchKernelGGL(lqr_riccati_kernel<false>, dim3(rows), dim3(64), 0, s, r);
        GPMPC_HIP_CHECK(h, hipGetLastError());
    }
    return GPMPC_OK;
}

}  // namespace gpmpc_hip
