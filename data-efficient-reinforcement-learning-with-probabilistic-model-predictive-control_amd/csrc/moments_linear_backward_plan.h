// moments_linear_backward_plan.h -- host-side planning of gpmpc_moments_linear_backward / gpmpc_rollout_linear_backward /
// gpmpc_rollout_linear_feedback_backward (moments_linear_backward.hip): how many points or candidates a chunk holds and where each array of its workspace starts.
// Plain C++ (no HIP), so that a stand-alone host program can run it under a sanitizer
// (tools/host_checks/moments_linear_backward_plan_check.cpp).
#pragma once
#include <cstddef>

#include "moments_linear_plan.h"

namespace gpmpc_hip {

constexpr int kLinBwdBM = kLinBM;                          // the forward's tile (one tile kernel serves both): query rows per workgroup
constexpr int kLinBwdBN = kLinBN;                          // ... and columns of iK per workgroup
constexpr size_t kLinBwdWsBudget = (size_t)16 << 20;       // bytes of workspace per chunk (or one 64-row tile's need if that is more)

struct LinearBwdPlan {
    int nCB;                 // column blocks of iK
    int NW;                  // values per (output, row): the forward's sums  sum P k | sum k beta | E sums beta k (x_j - m),
                             // the reverse pass's coefficients  M_bar_a | s_a | E weights W[e,a] / l_ae^2  and its E sums c k (x_j - m)
    long long chunk;         // points / candidates per chunk (>= 1)
    long long Mc;            // row stride of part / coef: chunk rounded up to the tile height
    // offsets (doubles) of the arrays of one chunk, in this order, and their sizes
    size_t part, n_part;     // (D, nCB, NW, Mc) partial sums of a tile launch
    size_t coef, n_coef;     // (D, NW, Mc) per-row coefficients of the reverse tile launch
    size_t base, n_base;     // (chunk, E) sum_a W[g,a] M_a / l_ag^2
    // rollout only (H >= 1)
    size_t xq, n_xq;         // (Mc, E) model inputs of the next tile launch
    size_t mu, n_mu;         // (chunk, H + 1, D) recomputed trajectory
    size_t Sig, n_Sig;       // (chunk, H + 1, D, D)
    size_t stepM, n_stepM;   // (chunk, H, D) every step's M
    size_t stepV, n_stepV;   // (chunk, H, D + KA, D) ... and the state rows of its V (closed loop: and the KA = A action rows)
    size_t cv, n_cv;         // (chunk, H + 1) cost variances of the recomputed trajectory
    size_t adj, n_adj;       // (chunk, 2 D + D D + A): lambda | Lambda | the step's cost partials wrt mu and the action
                             // (closed loop: gains_bar_t is complete when step t is opened -- nothing of it is parked here)
    size_t total;            // doubles
};

// count: points (H = 0: gpmpc_moments_linear_backward; A ignored) or candidates (H >= 1: gpmpc_rollout_linear_backward);
// opt_chunk: option "moments_linear_backward_chunk_points" (0 = auto); KA: action rows of V kept per step (0: open loop -- every
// offset and the chunk size are then what they were without the parameter; A: gpmpc_rollout_linear_feedback_backward).  Needs
// N, D, E >= 1, A >= 0, KA in {0, A} and count >= 1.
inline void plan_moments_linear_backward(int N, int D, int E, int A, long long count, int H, long long opt_chunk, int KA,
                                         LinearBwdPlan& p) {
    p.nCB = (N + kLinBwdBN - 1) / kLinBwdBN;
    p.NW = E + 2;
    const size_t DD = (size_t)D * D;
    const size_t adj_row = H > 0 ? 2 * (size_t)D + DD + (size_t)A : 0;
    size_t per_row = (size_t)D * p.nCB * p.NW + (size_t)D * p.NW + (size_t)E;
    if (H > 0) per_row += (size_t)E + (size_t)(H + 1) * ((size_t)D + DD) + (size_t)H * ((size_t)D + DD + (size_t)KA * D) + (size_t)(H + 1) + adj_row;
    long long chunk = (long long)(kLinBwdWsBudget / (sizeof(double) * per_row)) / kLinBwdBM * kLinBwdBM;
    if (opt_chunk > 0) chunk = opt_chunk;
    if (chunk < 1) chunk = kLinBwdBM;
    if (chunk > count) chunk = count;
    p.chunk = chunk;
    p.Mc = (chunk + kLinBwdBM - 1) / kLinBwdBM * kLinBwdBM;
    const size_t c = (size_t)chunk, Mc = (size_t)p.Mc;
    size_t o = 0;
    auto take = [&](size_t& off, size_t& n, size_t size) { off = o; n = size; o += size; };
    take(p.part, p.n_part, (size_t)D * p.nCB * p.NW * Mc);
    take(p.coef, p.n_coef, (size_t)D * p.NW * Mc);
    take(p.base, p.n_base, c * E);
    const bool roll = H > 0;
    take(p.xq, p.n_xq, roll ? Mc * E : 0);
    take(p.mu, p.n_mu, roll ? c * (H + 1) * D : 0);
    take(p.Sig, p.n_Sig, roll ? c * (H + 1) * DD : 0);
    take(p.stepM, p.n_stepM, roll ? c * H * D : 0);
    take(p.stepV, p.n_stepV, roll ? c * H * (DD + (size_t)KA * D) : 0);
    take(p.cv, p.n_cv, roll ? c * (H + 1) : 0);
    take(p.adj, p.n_adj, c * adj_row);
    p.total = o;
}

}  // namespace gpmpc_hip
